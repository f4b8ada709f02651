"""The spectral filter contraction (ace_amd/csrc/dhconv_strip.hip, C ABI `ace_dhconv_strip_op`) stated in plain torch from the reference,
the cases tests/test_gpu_dhconv_strip.py holds the kernel to, and their inputs.  tests/test_dhconv_ref_cpu.py holds this file itself.

    dense    out[b,o,l,m]   = sum_i x[b,i,l,m]   w[i,o,l]       einsum("bixy,iox->boxy")      contractions.py:183-195
    grouped  out[b,g,o,l,m] = sum_i x[b,g,i,l,m] w[g,l,o,i]     einsum("bgixy,gxoi->bgoxy")   conditional_sfno/s2convolutions.py:119-135

on complex values, the coefficients with m > l zeroed first (every SHT output has them zero; the kernel never reads them).

The metric is PER DEGREE: for each l, max |got_l - ref_l| / max |ref_l| over samples, channels and m <= l; a case's error is its worst
degree.  The inputs fall with l as real spectra do - coefficients (1 + l)^-2, filter (1 + l)^-1 / C - so under the whole-tensor
ratio max |err| / max |ref| (reported beside it) a wrong strip or a dropped low-order product in a weak degree would vanish under
degree 0.  OP_TOL = 2e-6, the operator bar of tests/test_gpu_parity.py, applies to the per-degree metric.

A case is (n, C, L, Mm, groups, storage, variant).  Rows of a degree are (m, sample): rows(l) = min((l + 1) n, Mm n); a workgroup
owns (l, 128 output channels, a chunk of up to 96 rows = 1 .. 3 strips of 32)."""

import dataclasses
import functools
import zlib

import torch

OP_TOL = 2e-6
DENSE, NATIVE = 0, 1
CHUNK_ROWS = 96


@dataclasses.dataclass(frozen=True)
class Case:
    family: str          # strips | chunks | cols | xcd | gdense | gnative | range
    n: int
    C: int
    L: int
    Mm: int
    groups: int = 1
    storage: int = DENSE
    variant: str = ""    # range family: which operand is scaled, and how

    @property
    def id(self):
        s = f"{self.family}-n{self.n}-C{self.C}-L{self.L}-Mm{self.Mm}"
        if self.groups > 1:
            s += f"-G{self.groups}-{'native' if self.storage == NATIVE else 'dense'}"
        return s + (f"-{self.variant}" if self.variant else "")

    @property
    def data_key(self):
        """cases with the same key have the same inputs and the same truth (the storage form is the library's business)"""
        return (self.n, self.C, self.L, self.Mm, self.groups, self.variant)


# the two-chunk, three-strip ragged shape: rows(l) = 5 (l + 1) = 5 .. 120 - one, two and three strips, ragged (70, 75, .. 95), a full
# chunk never, a second chunk of 4 .. 24 rows at row0 = 96 from l = 19 on
T_SHAPE = (5, 24, 25)
SMALL_SHAPE = (1, 5, 6)
GROUPS_DENSE = ((256, 4), (256, 2), (512, 2), (384, 2), (384, 4))
GROUPS_NATIVE = ((256, 8), (256, 4), (512, 4), (512, 2))
RANGE_VARIANTS = ("x1e-12", "x1e8", "w1e-6", "w1e4", "spike", "xmax2^-95", "xmax2^115")
RANGE_ENDS = ("xmax2^-95", "xmax2^115")   # where the host's unclamped and the kernel's clamped exponent parted: correct, or refused


def cases():
    out = [Case("strips", 1, 128, 96, 96)]                       # rows(l) = l + 1: every row count 1 .. 96 once
    out += [Case("chunks", 3, 128, 40, 41),                      # 3 .. 120 rows: a second chunk of 3 .. 24 rows
            Case("chunks", 5, 128, 40, 41),                      # 5 .. 200 rows: a third chunk at row0 = 192
            Case("chunks", 2, 128, 24, 10)]                      # rows capped at Mm n = 20 below (l + 1) n
    out += [Case("cols", *T_SHAPE[:1], C, *T_SHAPE[1:]) for C in (128, 256, 384, 512)]   # nstages 4, 8, 12, 16; column groups 0 .. 3
    out += [Case("xcd", 1, 128, L, L + 1) for L in (1, 5, 8, 9)]   # empty per-XCD lists, rows = 0 padding, L % 8 != 0
    for fam, lst, st in (("gdense", GROUPS_DENSE, DENSE), ("gnative", GROUPS_NATIVE, NATIVE)):
        for C, G in lst:
            for n, L, Mm in (T_SHAPE, SMALL_SHAPE):
                out.append(Case(fam, n, C, L, Mm, G, st))
    out += [Case("range", 3, 128, 24, 25, variant=v) for v in RANGE_VARIANTS]
    return out


def rows_of(case, l):
    return min((l + 1) * case.n, case.Mm * case.n)


def triangle(L, Mm):
    """(L, Mm) bool: m <= l"""
    return torch.arange(Mm)[None, :] <= torch.arange(L)[:, None]


def expected_route(case):
    """(storage, kspan, (units with 1, 2, 3 strips), max chunks of a (degree, column group)) restated from the kernel's contract"""
    cg = case.C // case.groups
    skip = case.groups > 1 and (cg % 128 == 0 or 128 % cg == 0)
    kspan = max(cg, 128) if skip else case.C
    hist, most = [0, 0, 0], 0
    for l in range(case.L):
        rows, nch = rows_of(case, l), 0
        for row0 in range(0, rows, CHUNK_ROWS):
            hist[(min(rows - row0, CHUNK_ROWS) + 31) // 32 - 1] += case.C // 128
            nch += 1
        most = max(most, nch)
    return case.storage, kspan, tuple(hist), most


def native_ok(C, G):
    return G > 1 and C % G == 0 and C % 128 == 0 and (C // G) % 32 == 0 and ((C // G) % 128 == 0 or 128 % (C // G) == 0)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    n, C, L, Mm, G, variant = key
    g = torch.Generator().manual_seed(zlib.crc32(repr(key[:5]).encode()))
    deg = torch.arange(L, dtype=torch.float32)
    x = torch.randn(n, C, L, Mm, 2, generator=g) * (1.0 + deg)[None, None, :, None, None] ** -2
    if G == 1:
        w = torch.randn(C, C, L, 2, generator=g) * ((1.0 + deg) ** -1 / C)[None, None, :, None]
    else:
        w = torch.randn(G, L, C // G, C // G, 2, generator=g) * ((1.0 + deg) ** -1 / C)[None, :, None, None, None]
    x = x * triangle(L, Mm)[None, None, :, :, None]
    if variant.startswith("x1e"):
        x = x * float(variant[1:])
    elif variant.startswith("w1e"):
        w = w * float(variant[1:])
    elif variant == "spike":           # the largest coefficient in one element only: one shard word of the range slot carries the bound
        x[n - 1, C - 3, 0, 0, 1] = 4.0 * float(x.abs().max())
    elif variant.startswith("xmax2^"):   # ... and that element an exact power of two, everything else below a quarter of it
        top = 2.0 ** int(variant[6:])
        x = x * (top / 4.0 / float(x.abs().max()))
        x[n - 1, C - 3, 0, 0, 1] = top
    elif variant:
        raise ValueError(variant)
    return x.contiguous(), w.contiguous()


def inputs(case):
    """(coefficients (n, C, L, Mm, 2) with m > l zero, filter (C, C, L, 2) or (G, L, C/G, C/G, 2)), fp32, shared: do not modify"""
    return _inputs(case.data_key)


def contract(x, w, groups, dtype):
    """the reference's einsum at `dtype` (torch.float64 or torch.float32) -> complex (n, C, L, Mm)"""
    n, C, L, Mm, _ = x.shape
    xc = torch.view_as_complex((x.to(dtype) * triangle(L, Mm)[None, None, :, :, None]).contiguous())
    wc = torch.view_as_complex(w.to(dtype).contiguous())
    if groups == 1:
        return torch.einsum("bixy,iox->boxy", xc, wc)
    xg = xc.reshape(n, groups, C // groups, L, Mm)
    return torch.einsum("bgixy,gxoi->bgoxy", xg, wc).reshape(n, C, L, Mm)


def expand_grouped(w, C, G):
    """(G, L, C/G [out], C/G [in], 2) -> the dense (C [in], C [out], L, 2) with exact zeros between groups"""
    cg = C // G
    dense = torch.zeros(C, C, w.shape[1], 2, dtype=w.dtype)
    for g in range(G):
        dense[g * cg:(g + 1) * cg, g * cg:(g + 1) * cg] = w[g].permute(2, 1, 0, 3)   # (L, o, i, 2) -> (i, o, L, 2)
    return dense


@functools.lru_cache(maxsize=None)
def _truth(key):
    x, w = _inputs(key)
    return contract(x, w, key[4], torch.float64)


def truth(case):
    """fp64, complex (n, C, L, Mm); zero where m > l.  Shared: do not modify"""
    return _truth(case.data_key)


def degree_errors(got, ref):
    """(worst per-degree error, the degree, whole-tensor max |err| / max |ref|); got, ref complex (n, C, L, Mm), compared on m <= l"""
    L, Mm = ref.shape[2], ref.shape[3]
    tri = triangle(L, Mm)[None, None]
    err = ((got.to(torch.complex128) - ref).abs() * tri).amax(dim=(0, 1, 3))
    mag = (ref.abs() * tri).amax(dim=(0, 1, 3))
    assert float(mag.min()) > 0.0, "a degree with a zero reference"
    per = err / mag
    l = int(per.argmax())
    return float(per[l]), l, float(err.max() / mag.max())
