"""NumPy restatement of the sample generator every batched RANSAC stage shares (k_ransac_samples in
sfm_amd/csrc/ransac_kernels.h; the rule is written out above draw_distinct<N> in ransac_common.h)."""
import numpy as np

MAX_DRAWS = 256
_U = np.uint64


def mix64(z):
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def draw_samples(seed, segment, n_points, n_hyp, size, min_points):
    """[n_hyp, size] int32: the samples the device draws for segment `segment` holding `n_points` points (all -1 when
    it has fewer than min_points).  A function of (seed, segment, hypothesis) and n_points only."""
    out = np.full((n_hyp, size), -1, dtype=np.int32)
    if n_points < min_points:
        return out
    hyp = np.arange(n_hyp, dtype=np.uint64)
    key = mix64(mix64(mix64(np.array([seed], dtype=np.uint64)) ^ _U(segment)) ^ hyp)
    d = np.zeros(n_hyp, dtype=np.uint64)
    for k in range(size):
        pending = np.ones(n_hyp, dtype=bool)
        while True:
            pending &= d < MAX_DRAWS
            if not pending.any():
                break
            i = np.flatnonzero(pending)
            c = (((mix64(key[i] ^ d[i]) >> _U(32)) * _U(n_points)) >> _U(32)).astype(np.int32)
            d[i] += _U(1)
            dup = (out[i, :k] == c[:, None]).any(axis=1)
            out[i[~dup], k] = c[~dup]
            pending[i[~dup]] = False
        for h in np.flatnonzero(out[:, k] < 0):          # draws exhausted: the lowest unused index
            out[h, k] = min(set(range(size)) - set(out[h, :k].tolist()))
    return out
