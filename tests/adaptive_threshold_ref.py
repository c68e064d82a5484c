"""numpy restatement of adaptive sampling's selection by threshold and of the driver built on it (include/pt_amd.h
pt_adaptive_round_threshold, pt_render_threshold; csrc/pt_adaptive.h), on top of adaptive_ref.keys: the key does not change.
pt_adaptive_select_threshold_host and the device's kernels must equal select_threshold in list, above and m; a whole run must equal
simulate, bit for bit, when it is fed the renderer's own samples."""
import numpy as np

import adaptive_ref
import noise_ref
from adaptive_ref import bits, f32  # noqa: F401


def threshold_bits(threshold):
    """bits(thr), thr = threshold * threshold in ONE float32 multiply."""
    with np.errstate(all="ignore"):
        return int(bits(np.array([f32(threshold) * f32(threshold)], f32))[0])


def select_threshold(w, W, R, counts, threshold, cap):
    """(list int32 [m] ascending, above, m): the pixels whose key bits exceed bits(thr), the `cap` with the largest keys at the
    most, equal keys by the smaller tile index."""
    k = adaptive_ref.keys(w, W, R, counts)
    is_above = k > np.uint32(threshold_bits(threshold))
    above = int(is_above.sum())
    m = min(above, int(cap))
    if above <= cap:
        return np.flatnonzero(is_above).astype(np.int32), above, m
    order = np.lexsort((np.arange(k.size), -k.astype(np.int64)))  # key descending, then index ascending
    return np.sort(order[:m]).astype(np.int32), above, m


def case_thresholds(w, W, R, counts):
    """{name: threshold} for one made-up tile: 0; below the smallest non-zero key; one whose square IS a key (only where a key is an
    exact float32 square: the tie is not above); between two keys; above the largest (an empty list)."""
    k = adaptive_ref.keys(w, W, R, counts)
    vals = np.unique(k[k != 0xFFFFFFFF]).view(f32)
    out = {"zero": 0.0}
    pos = vals[vals > 0]
    if pos.size:
        out["below"] = float(np.sqrt(pos[0].astype(np.float64)) * 0.5)
        out["past"] = float(np.sqrt(pos[-1].astype(np.float64)) * 2.0 + 1.0)
        mid = pos[pos.size // 2]
        root = f32(np.sqrt(mid.astype(np.float64)))
        if pos.size > 1:
            lo, hi = pos[pos.size // 2 - 1], mid
            between = f32(np.sqrt((lo.astype(np.float64) + hi.astype(np.float64)) / 2))
            if lo <= f32(between * between) < hi:
                out["between"] = float(between)
        if f32(root * root) == mid:
            out["tie"] = float(root)
    else:
        out["past"] = 1.0
    return out


def caps(n):
    return sorted({1, -(-n // 4), n})


def check(select, planes, counts, W, R, threshold, cap, what):
    """`select` (the host or the stage function) against the restatement; returns (above, m)."""
    want, above, m = select_threshold(planes[0, :, 3], W, R, counts, threshold, cap)
    got, got_above, got_m = select(planes, counts, W, R, threshold, cap)
    assert (got_above, got_m) == (above, m) and m == min(above, cap), (what, got_above, got_m, above, m)
    assert np.array_equal(got, want), (what, got[:8], want[:8])
    assert m < 2 or np.all(np.diff(got) > 0), what  # ascending tile index, distinct
    if above > cap:  # bit for bit the list of the existing top-cap selection
        assert np.array_equal(got, adaptive_ref.select(planes[0, :, 3], W, R, counts, cap)), what
    return above, m


def tie_pattern(name, W, R):
    """(planes, counts, threshold) with many keys EXACTLY equal to threshold^2: adaptive_ref's `three` at half its values (bands of
    0.125, 0.25, 0.5; inside a band the key is the band's value exactly) with the threshold 0.5 on the middle band, so that the
    refused ties straddle waves and blocks; `equal` with every estimate 0.25, where nothing is above 0.5."""
    planes, counts = adaptive_ref.pattern(name, W, R)
    if name == "three":
        planes[0, :, 3] = (planes[0, :, 3] * f32(0.5)).astype(f32)
    elif name == "equal":
        planes[0, :, 3] = f32(0.25)
    else:
        raise KeyError(name)
    return planes, counts, 0.5


def simulate(W, R, group_sum, G, threshold, max_fraction, max_rounds, min_pixels=0, warm_up=2):
    """The driver on samples from `group_sum(first, count)` -> float32 [n, 3], the sum of those iterations for every tile pixel
    starting from zero, added in iteration order.  warm_up uniform groups of G with a fold each (iterations 1 ...; the image
    accumulates across them as the renderer's does, so group_sum(first, count, accum) continues a sum), then rounds of G over the
    threshold list until at most min_pixels are above or max_rounds rounds ran.
    Returns dict(S, planes, counts, lengths [rounds], above [rounds + 1 or rounds], samples, iters)."""
    n = W * R
    cap = adaptive_ref.list_length(max_fraction, n)
    planes = noise_ref.new_planes(n)
    S, T = None, 0
    for M in range(1, warm_up + 1):
        S = group_sum(T + 1, G, S)
        T += G
        noise_ref.fold(S, planes, G, M, T)
    S = S.copy()
    counts = adaptive_ref.uniform_counts(n, T, warm_up)
    lengths, aboves, samples = [], [], warm_up * G * n
    while len(lengths) < max_rounds:
        lst, above, m = select_threshold(planes[0, :, 3], W, R, counts, threshold, cap)
        aboves.append(above)
        if above <= min_pixels:
            break
        Sw = group_sum(T + 1, G, None)[lst]
        adaptive_ref.merge(S, planes, counts, lst, Sw, G)
        T += G
        lengths.append(m)
        samples += G * m
    return dict(S=S, planes=planes, counts=counts, lengths=lengths, above=aboves, samples=samples, iters=T)


def uniform_groups_to_criterion(W, R, group_sum, G, threshold, max_groups, min_pixels=0):
    """Uniform sampling in groups of G with a fold each: the number of groups after which at most min_pixels pixels are above the
    threshold (None when max_groups do not get there), and the SUM images after every group."""
    n = W * R
    planes = noise_ref.new_planes(n)
    S, T, sums = None, 0, []
    for M in range(1, max_groups + 1):
        S = group_sum(T + 1, G, S)
        T += G
        noise_ref.fold(S, planes, G, M, T)
        sums.append(S.copy())
        if M >= 2 and select_threshold(planes[0, :, 3], W, R, adaptive_ref.uniform_counts(n, T, M), threshold, n)[1] <= min_pixels:
            return M, sums
    return None, sums
