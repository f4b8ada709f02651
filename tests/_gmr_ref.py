"""TEST INFRASTRUCTURE: the numpy statement of the global-mean-removal contract of include/ace_sfno.h ("Global-mean removal") -
the partial sums in the stated order, sample mean, shift, pack, synthetic channels and unpack with the stated roundings, every
fp32 operation one ``np.float32`` operation at a time.  csrc/gmr.hip is held to it bit for bit (tests/test_gpu_gmr_kernels.py),
tests/_fake_gmr.py emulates the C entries with it, and tests/test_gmr_ref_cpu.py holds the statement itself to exact sums and to
the torch ops of the reference's formulas."""
import numpy as np

CHUNK = 4096        # pixels per partial sum
NT = 256            # accumulator groups: pixel i of a chunk -> accumulator i % 4 of group (i // 4) % NT, round i // (4 NT)
ROUNDS = CHUNK // (4 * NT)


def chunks(hw: int) -> int:
    return (hw + CHUNK - 1) // CHUNK


def chunk_sum(x: np.ndarray) -> np.float64:
    """one partial: x holds the n <= CHUNK fp32 pixels of the chunk"""
    assert x.dtype == np.float32 and 0 < x.size <= CHUNK
    full = np.zeros(CHUNK, dtype=np.float64)            # a pixel past n counts as +0.0
    full[:x.size] = x.astype(np.float64)
    v = full.reshape(ROUNDS, NT, 4)                     # [r][t][q] = x[4 (NT r + t) + q]
    a = np.zeros((NT, 4), dtype=np.float64)
    for r in range(ROUNDS):                             # rounds ascending, from +0.0
        a = a + v[r]
    s = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])
    s = s.reshape(NT // 64, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):                    # the lanes of a group of 64
        s[:, :off] = s[:, :off] + s[:, off:2 * off]
    w = s[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def partials(plane: np.ndarray) -> np.ndarray:
    """fp64 [chunks(hw)] of one (sample, plane) of hw fp32 pixels"""
    x = np.ascontiguousarray(plane, dtype=np.float32).reshape(-1)
    return np.array([chunk_sum(x[c * CHUNK:(c + 1) * CHUNK]) for c in range(chunks(x.size))], dtype=np.float64)


def sample_mean(plane: np.ndarray) -> np.float32:
    """the partials added in chunk order, one fp64 division by hw, one rounding to fp32"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = partials(plane)
        s = p[0]
        for c in range(1, p.size):
            s = s + p[c]
        return np.float32(s / np.float64(np.asarray(plane).size))


def shift_of(clim_mean, plane: np.ndarray) -> np.float32:
    """global_mean_removal.py:231 / :316: means[field] - sample_mean in fp32"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(clim_mean) - sample_mean(plane)


def pack(src: np.ndarray, shift, mean, std) -> np.ndarray:
    """((src + shift) - mean) / std, three roundings; shift None: the plain (src - mean) / std"""
    src = np.asarray(src, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if shift is not None:
            src = src + np.float32(shift)
        return (src - np.float32(mean)) / np.float32(std)


def extra(shift, std) -> np.float32:
    """the synthetic channel's value: (-shift) / std"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return (-np.float32(shift)) / np.float32(std)


def unpack(y: np.ndarray, shift, mean, std) -> np.ndarray:
    """(y * std + mean) - shift, the product rounded before the sum; shift None: the plain y * std + mean"""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = y * np.float32(std)
        q = p + np.float32(mean)
        return q if shift is None else q - np.float32(shift)
