"""CPU restatement of ops.window_weights (include/floodseg_test.h, window_weights): the per-frame blend weights of one key-frame
window from the cut flags of its frame pairs.  The window has frames 0..n (0 = the previous key frame, n = the next one, not emitted);
cuts[j-1] is the flag of the pair (j-1 -> j), j = 1..n, None meaning "not estimated: no cut"."""
import numpy as np

BLENDED, HELD_PREV, HELD_NEXT, BETWEEN_CUTS = 0, 1, 2, 3


def window_weights(cuts, n):
    """(weights float32 [n,2], source int32 [n])."""
    cuts = list(cuts)
    assert n >= 1 and len(cuts) == n
    where = [j for j in range(1, n + 1) if cuts[j - 1]]
    weights = np.empty((n, 2), dtype=np.float32)
    source = np.empty((n,), dtype=np.int32)
    for f in range(n):
        if not where:
            weights[f] = (np.float32(np.float64(n - f) / np.float64(n)), np.float32(np.float64(f) / np.float64(n)))
            source[f] = BLENDED
        elif f < where[0]:
            weights[f], source[f] = (1.0, 0.0), HELD_PREV
        elif f >= where[-1]:
            weights[f], source[f] = (0.0, 1.0), HELD_NEXT
        else:
            weights[f], source[f] = ((1.0, 0.0) if 2 * f <= n else (0.0, 1.0)), BETWEEN_CUTS
    return weights, source
