"""The inputs of the large-frame tests (tests/test_large_frames_host.py on the CPU, tests/test_gpu_large_frames.py on the device): frames,
lists and planes just past the sizes at which a post-processing kernel takes another path.  Plain numpy on top of the *_ref modules.

  k_noise_reduce (csrc/pt_noise.hip)          adds the per-1,024-pixel partial sums CHUNK = 1,024 at a time: a second chunk above
                                              1,048,576 pixels
  k_adaptive_scan (csrc/pt_adaptive.hip),     scan one count per workgroup of BLOCK = 1,024 pixels or list entries, PASS = 256 workgroups
  k_partition_scan (csrc/pt_group_select.hip) per pass with a carry between passes: a second pass above 262,144 pixels or entries
  level_slots, first_row (csrc/pt_denoise.h)  map level l of the à-trous filter onto groups of kRows << l = 4 << l rows: more than one
                                              group at levels 4 .. 7 needs more than 64 .. 512 rows
"""
import numpy as np

import adaptive_ref
import adaptive_threshold_ref
import denoise_adaptive_ref
import denoise_guided_ref
import denoise_ref
import history_moments_ref
import history_noise_ref
import history_round_ref
import history_threshold_ref

f32 = np.float32
BLOCK = 1024  # pixels or list entries of one workgroup, and of one partial sum
PASS = 256    # workgroups per pass of the scans
CHUNK = 1024  # partial sums per chunk of the reduce


def blocks(entries):
    return -(-int(entries) // BLOCK)


# ---- 1. the reduce over more than one chunk ------------------------------------------------------------------------------------------
# pixels, partial sums: one chunk exactly full | a second chunk of one partial | a third chunk of two, the last workgroup with 5 pixels
REDUCE_PIXELS = ((1024 * 1024, 1024), (1025 * 1024, 1025), (2049 * 1024 + 5, 2050))
SPIKE_SPANS = (0, 1023, 1024, 2047, 2048, 2049)  # the partials at both ends of every chunk of the largest size
REDUCE_GROUPS, REDUCE_ITERS, REDUCE_SAMPLES = 2, 2, 2.0
REDUCE_UNIT = 2.0 ** -9  # every estimate, and so every sum of them, is a multiple of this


def summable_planes(npix, seed=0):
    """The fold's planes [2, npix, 4] whose estimates add up exactly: plane 0 zero, q = integers in [0, 4096) times 2^-8.  With M = 2,
    T = 2, samples = 2 and no history the estimate is w = (q.x / 2 + q.y / 2) + q.z / 2, a multiple of 2^-9 below 24, exact in float32;
    a double holds every sum of 2.1 million of them (below 2^35 units of 2^-9) exactly, so the order of the additions cannot show."""
    rng = np.random.default_rng(4099 * seed + npix)
    planes = np.zeros((2, npix, 4), f32)
    planes[1, :, :3] = rng.integers(0, 4096, (npix, 3)).astype(f32) * f32(2.0 ** -8)
    return planes


def span_of(npix, span):
    """The pixels of partial sum `span`."""
    return slice(span * BLOCK, min((span + 1) * BLOCK, npix))


def uniform_counts(npix):
    """Counts (T_p, M_p) = (2, 2) for every pixel: the counted form's divisors are then the uniform form's, Tf = Df = 2."""
    return adaptive_ref.uniform_counts(npix, REDUCE_ITERS, REDUCE_GROUPS)


exact_sum = history_noise_ref.exact_sum


# ---- 2. selection with more than one scan pass ---------------------------------------------------------------------------------------
# W, R, workgroups: one pass, full | the second pass holds one workgroup | the third holds two, the last ragged (833 pixels)
SELECT_FRAMES = ((512, 512, 256), (513, 512, 257), (1025, 513, 514))
SELECT_PATTERNS = ("random", "equal", "three", "mixedT")
THRESHOLD_FRAMES = SELECT_FRAMES[1:]
THRESHOLD_PATTERNS = ("random", "three")
NAN_FRAME = (513, 512)
NAN_PIXELS = (5, 262150)  # one in each pass of the scan (workgroups 0 and 256)
NAN_LENGTHS = (1, 15, 300)


def nan_planes():
    """The two-NaN case of test_gpu_adaptive_select.py at NAN_FRAME; each NaN poisons the keys of its 3 x 3 neighbourhood (six keys: both
    lie in a border row)."""
    W, R = NAN_FRAME
    planes, counts = adaptive_ref.pattern("random", W, R)
    planes[0, NAN_PIXELS[1], 3] = np.nan
    planes[0, NAN_PIXELS[0], 3] = -np.nan
    return planes, counts


def threshold_caps(n):
    return (1, n // 4, n)


def threshold_case(name, W, R):
    """(planes, counts, {name: threshold}) of adaptive_ref's pattern with adaptive_threshold_ref's thresholds."""
    planes, counts = adaptive_ref.pattern(name, W, R)
    return planes, counts, adaptive_threshold_ref.case_thresholds(planes[0, :, 3], W, R, counts)


def blend_select_case(W, R):
    """The inputs of one selection by threshold over the blend, as test_gpu_history_threshold.py builds them: random counts, the planes a
    render with them could have left, C and VC present; the threshold between two keys, the cap a quarter of the frame."""
    n = W * R
    counts = history_threshold_ref.random_counts(n)
    noise, _ = history_threshold_ref.noise_planes(counts)
    Cp, VC = history_threshold_ref.current_planes(n, 3 * n)
    thr = history_threshold_ref.thresholds(noise, counts, W, R, Cp, VC)
    return noise, counts, Cp, VC, thr.get("between", thr["below"]), n // 4


def history_select_case(W, R):
    """(feature planes, current plane, emitter table) of test_gpu_history_round.py's stage test."""
    feat, Cp = history_round_ref.random_planes(W, R)
    return feat, Cp, history_round_ref.EMITTER


# ---- 3. partition with more than one scan pass ---------------------------------------------------------------------------------------
PARTITION_PARTS = (2, 3, 64)  # 64 = kMaxParts


def partition_lists(n):
    """(name, w, h, ascending int32 list, its workgroups) for n contexts.  `part 0 only` holds whole rows y with y % n == 0, so that every
    other part counts zero in every workgroup of every pass: 512 rows of 1025 x 1024 for n = 2 (524,800 entries), 342 for n = 3, and for
    n = 64 the 257 such rows of a frame of 16,385 rows."""
    every = lambda w, h: np.arange(w * h, dtype=np.int32)  # noqa: E731
    out = [("every pixel of 512 x 512", 512, 512, every(512, 512), 256),
           ("every pixel of 513 x 512", 513, 512, every(513, 512), 257),
           ("every pixel of 1025 x 513", 1025, 513, every(1025, 513), 514)]
    rng = np.random.default_rng(5 + 1000 * n)
    out.append(("270,000 of 513 x 600", 513, 600, np.sort(rng.choice(513 * 600, 270000, replace=False)).astype(np.int32), 264))
    w, h = (1025, 1024) if n < 64 else (1025, 64 * 256 + 1)
    rows = np.arange(0, h, n, dtype=np.int64)
    lst = (rows[:, None] * w + np.arange(w, dtype=np.int64)[None, :]).reshape(-1).astype(np.int32)
    out.append(("part 0 only", w, h, lst, blocks(lst.size)))
    return out


# ---- 4. à-trous levels with several row groups and more than two x tiles ----------------------------------------------------------------
DENOISE_FRAME = (130, 521)  # two full 64-wide tiles and one of two lanes; 9, 5, 3, 2 row groups at levels 4, 5, 6, 7
DENOISE_SPP = 4
OFF = dict(sigma_color=-1.0, sigma_normal=-1.0, sigma_position=-1.0)
# the four option sets of test_gpu_denoise.py's test_stage_equals_host, and all eight levels with every edge-stopping term off: the
# weights are then the stencil's own, so every tap of every level carries weight into the result (random_frame's neighbours are far
# apart in normal and position: under the default sigmas a distant tap weighs ~1e-20 of the centre)
PLAIN_OPTIONS = (dict(), dict(levels=8), dict(levels=3, keep_albedo=True), dict(levels=2, **OFF), dict(levels=8, **OFF))
RESTATED_OPTIONS = (dict(levels=8), dict(levels=8, **OFF))  # what the numpy restatement is asked on the CPU
GUIDED_GROUPS, GUIDED_ITERS = 3, 7
MOMENTS_SPP = 1


def group_counts(rows, level, k_rows=4):
    """Row groups of a level: ceil(rows / (kRows << level))."""
    return -(-rows // (k_rows << level))


def plain_inputs():
    w, rows = DENOISE_FRAME
    return denoise_ref.random_frame(w, rows, DENOISE_SPP)


def guided_inputs():
    """(rgb, feature planes, noise planes) as test_gpu_denoise_guided.py's stage test builds them."""
    w, rows = DENOISE_FRAME
    _, planes = denoise_ref.random_frame(w, rows, GUIDED_ITERS)
    noise = denoise_guided_ref.random_noise_planes(w, rows, GUIDED_GROUPS, GUIDED_ITERS)
    return np.ascontiguousarray(noise[0, :, :3]), planes, noise


def adaptive_inputs():
    """guided_inputs and heterogeneous counts, as test_gpu_denoise_adaptive.py's stage test builds them."""
    w, rows = DENOISE_FRAME
    return guided_inputs() + (denoise_adaptive_ref.random_counts(w, rows),)


def moments_inputs():
    """(S, feature planes, C, VC) as test_gpu_history_moments.py's stage test builds them, the marks in a checkerboard: the spatial
    estimate and the temporal branch alternate in every wave."""
    w, rows = DENOISE_FRAME
    S, planes = denoise_ref.random_frame(w, rows, MOMENTS_SPP)
    Cp, VC, _ = history_moments_ref.current_planes(w, rows, "checkerboard")
    return S, planes, Cp, VC


# ---- 5. one renderer case at a frame with more than 1,024 partials ----------------------------------------------------------------------
RENDER_RES = (1025, 1024)  # 1,025 partial sums: the reduce's second chunk holds one
RENDER_FRACTION = 1.0 / 64
SSE_RTOL = 1e-9  # the suite's bound on an SSE; summing n non-negative doubles in any order is within (n - 1) 2^-53 = 1.2e-10 here
