"""The step guard (include/emdr2_ops.h, "Step guard") restated in numpy: the census of the non-finite elements that rides in the norm pass
and the transitions of the guard's eight state words.  Plain integer arithmetic on Python ints; the device kernels must give exactly this."""
import numpy as np

NO_KEY = (1 << 64) - 1
CENSUS_EMPTY = [0, 0, NO_KEY, 0]


def census(g, bucket=0, prior=None):
    """[NaN count, Inf count, min((bucket << 40) | index) over the non-finite elements, 0], merged into `prior` (another bucket's)."""
    g = np.asarray(g, dtype=np.float32)
    c = list(prior) if prior is not None else list(CENSUS_EMPTY)
    nan, inf = np.isnan(g), np.isinf(g)
    c[0] += int(nan.sum())
    c[1] += int(inf.sum())
    bad = np.flatnonzero(nan | inf)
    if bad.size:
        c[2] = min(c[2], (int(bucket) << 40) | int(bad[0]))
    return c


def verdict(gnorm_sq, census_words, state, step):
    """One emdr2_step_verdict: -> (new state words, the census as the kernel leaves it).  Skipped exactly when the fp32 norm is NaN or Inf."""
    s = list(state)
    skipped = not np.isfinite(np.float32(gnorm_sq))
    s[0] = int(skipped)
    if skipped:
        s[1] += 1
        s[2] += 1
        s[3] = max(s[3], s[2])
        if s[4] == 0:
            s[4], s[5], s[6], s[7] = int(step), census_words[2], census_words[0], census_words[1]
    else:
        s[2] = 0
    return s, list(CENSUS_EMPTY)


def words(t):
    """A device / host int64 tensor or array of uint64 bit patterns as Python ints."""
    return [int(x) & NO_KEY for x in (t.tolist() if hasattr(t, "tolist") else t)]
