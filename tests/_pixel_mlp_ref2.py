"""TEST INFRASTRUCTURE: the statement of ``ace_pixel_mlp_create2`` (include/ace_sfno.h) - tests/_pixel_mlp_ref.py's chain with the
embedding added BEFORE the activation of its layer when ``embed_before_act`` - in numpy, bit for bit for activations none and ReLU.
GELU and SiLU are not stated bit for bit: a layer with one of them must be the last one asked for, and ``pre_activation=True``
returns its accumulator (bias, fmaf chain, the embedding if it comes first) for an fp64 activation in the test."""
import numpy as np

from _pixel_mlp_ref import fmaf, k_order, relu

ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3


def pixel_mlp2(x, weights, biases, acts, embed_layer=-1, embed=None, embed_before_act=False, pre_activation=False):
    """x [B][dims[0]][hw] fp32; weights[l] [O][K]; biases[l] [O] or None; acts[l] ACT_*; embed [dims[embed_layer + 1]][hw]."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    B, _, hw = a.shape
    last = len(weights) - 1
    for l, w in enumerate(weights):
        w = np.asarray(w, dtype=np.float32)
        O, K = w.shape
        assert a.shape[1] == K
        bias = np.zeros(O, np.float32) if biases is None or biases[l] is None else np.asarray(biases[l], dtype=np.float32)
        acc = np.broadcast_to(bias[None, :, None], (B, O, hw)).copy()
        for k in k_order(K):
            acc = fmaf(np.broadcast_to(w[None, :, k, None], acc.shape), np.broadcast_to(a[:, None, k, :], acc.shape), acc)
        first = l == embed_layer and embed_before_act
        if first:
            with np.errstate(all="ignore"):
                acc = (acc + np.asarray(embed, dtype=np.float32)[None]).astype(np.float32)
        if acts[l] in (ACT_GELU, ACT_SILU) or (pre_activation and l == last):
            assert l == last and pre_activation and (first or l != embed_layer), "a soft activation is not stated bit for bit"
            return acc
        if acts[l] == ACT_RELU:
            acc = relu(acc)
        if l == embed_layer and not first:
            with np.errstate(all="ignore"):
                acc = (acc + np.asarray(embed, dtype=np.float32)[None]).astype(np.float32)
        a = acc
    return a
