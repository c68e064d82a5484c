"""shadeAndExtendRays (src/pathtrace.cu:336-437) for a live path, restated in numpy: every integer and float32 DECISION as the
kernels and the oracle make it, everything continuous in float64 from the float32 inputs.  The yardstick of the fma / fast
shading tests (tests/test_gpu_shade_modes.py); pinned to the oracle on the CPU by tests/test_shade_ref64_host.py, which also
measures the constants below.

Decisions kept in their own arithmetic: the seed utilhash((1 << 31) | depth << 22 | iter) ^ utilhash(pixel); minstd_rand's state
from its constructor; u01 = float32(x - 1) * 2^-31; the draws in the reference's order (roulette if depth > 3, the specular choice
if reflective > 0, then r1, r2, r3); emittance > 0; u > q; u < reflectivity; roughness = 1.0f - refractive > 0.
Continuous, float64: reflect, the local frame, ct = sqrt(1 - r1), st = sqrt(1 - ct^2), the specular angle roughness r1 pi / 2,
sin / cos(2 pi r), normalize(t x + f y + b z), the origin hp + 0.001f hn, the colour products and sky^(D - depth).
The frame's branch |f.x| > |f.y| is decided in float64; `frame_margin` = | |f.x| - |f.y| | lets a test leave the samples out whose
float32 axis could decide otherwise (only a reflected axis can: a diffuse one is the float32 normal itself)."""
import numpy as np

# ---- what tests/test_shade_ref64_host.py measured (2 math modes x (4 x 50,000 synthetic samples on cornell's materials + the
# ---- 2,000-odd golden vectors on ref_shade.txt), this file's inputs; the test re-measures and asserts <= these) -----------------
# the oracle's angle to the float64 direction in units of sigma = 2^-24 (1 + ct / st) (diffuse), 2^-24 (specular, mirror)
ORACLE_DIFFUSE_MAX = 4.8     # measured 4.75 in both math modes (114,237 samples)
ORACLE_SPECULAR_MAX = 8.8    # measured 8.71 (PORTABLE), 7.31 (LIBM) (39,728 samples): the float32 reflect() and frame; median of all 0.61
ORACLE_DIR_NORM_MAX = 1.8e-7    # | |dir| - |dir64| |, measured 1.77e-7
ORACLE_ORIGIN_ERR_MAX = 7.6e-8  # |origin - origin64| / max(|hp_k|, 1e-3) per component, measured 7.52e-8
# v_sin_f32 / v_cos_f32 on revolutions, the largest absolute error over every value a draw can return and over the lobe angles
# (pt_selfcheck_fast_math kinds 3-6, measured on an MI355X by tests/test_gpu_fast_math_blocks.py, which checks this pin)
TAU_HW = 1.45e-7  # measured 1.447e-7 (cos of the lobe angle; azimuth 1.254e-7), MI355X, 2026-10-20
FRAME_MARGIN = 1e-4          # samples with | |f.x| - |f.y| | below it are left out of the direction comparison only
FRAME_LEFT_OUT_CAP = 0.01

U24 = 2.0 ** -24
F001 = float(np.float32(0.001))


def utilhash(a):
    a = np.asarray(a).astype(np.uint32)
    with np.errstate(over="ignore"):
        a = (a + np.uint32(0x7ed55d16)) + (a << np.uint32(12))
        a = (a ^ np.uint32(0xc761c23c)) ^ (a >> np.uint32(19))
        a = (a + np.uint32(0x165667b1)) + (a << np.uint32(5))
        a = (a + np.uint32(0xd3a2646c)) ^ (a << np.uint32(9))
        a = (a + np.uint32(0xfd7046c5)) + (a << np.uint32(3))
        a = (a ^ np.uint32(0xb55a4f09)) ^ (a >> np.uint32(16))
    return a


def seed(it, depth, pixel):
    word = np.uint32(1 << 31) | np.uint32((int(depth) << 22) & 0xffffffff) | np.asarray(it).astype(np.uint32)
    return utilhash(word) ^ utilhash(np.asarray(pixel).astype(np.uint32))


class MinStd:
    """thrust::minstd_rand over arrays; draw(mask) advances only the masked engines."""
    M = np.uint64(2147483647)

    def __init__(self, s):
        r = s.astype(np.uint64) % self.M
        self.x = np.where(r == 0, np.uint64(1), r)

    def draw(self, mask=None):
        nx = (self.x * np.uint64(48271)) % self.M
        if mask is not None:
            nx = np.where(mask, nx, self.x)
        self.x = nx
        return ((nx - np.uint64(1)).astype(np.uint32).astype(np.float32) * np.float32(2.0 ** -31)).astype(np.float32)


def materials(arr) -> dict:
    """OrcMaterial / PtMaterial records as float32 arrays."""
    f = lambda k: np.array([getattr(m, k) for m in arr], np.float32)
    return dict(color=np.array([list(m.color) for m in arr], np.float32), spec=np.array([list(m.specular_color) for m in arr], np.float32),
                reflective=f("hasReflective"), refractive=f("hasRefractive"), emittance=f("emittance"))


def _norm(v):
    return v / np.sqrt((v * v).sum(axis=0, keepdims=True))


def angle(a, b):
    """Angle between the columns of a and b [3, n], float64, accurate for tiny angles."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b, axis=0), axis=0), (a * b).sum(axis=0))


def frame(f):
    """createLocalCoordinateSystem (pathtrace.cu:216-223) around the columns of f, float64: tangent, bitangent, margin."""
    a = np.abs(f[0]) > np.abs(f[1])
    z = np.zeros_like(f[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(a, _norm(np.stack([f[2], z, -f[0]])), _norm(np.stack([z, -f[2], f[1]])))
    return t, np.cross(f, t, axis=0), np.abs(np.abs(f[0]) - np.abs(f[1]))


def sky64(d):
    t = 0.5 * (d[1] + 1.0)
    w = 1.0 - t
    k = [float(np.float32(x)) for x in (0.5, 0.7, 1.0)]
    return np.stack([(w + t * k[0]) * 0.5, (w + t * k[1]) * 0.5, (w + t * k[2]) * 0.5])


def shade(mats: dict, trace_depth: int, depth: int, it, pixel, hit: dict, d, color) -> dict:
    """One step for n live paths.  Returns
      miss, kind (0 retired / 1 specular / 2 diffuse), alive (kind > 0 and depth + 1 < trace_depth: the stage's flag),
      color [3, n] float64 (a miss carries sky^(trace_depth - depth)), origin, dir [3, n] float64 (where kind > 0),
      sigma (the direction's unit of error, 2^-24 (1 + ct / st) diffuse, 2^-24 otherwise), sx (the sine that multiplies the
      azimuth's sin / cos: st or sin(angle)), perturbed, frame_margin, r (the three direction draws)."""
    n = len(it)
    d64, c64 = np.asarray(d, np.float64), np.asarray(color, np.float64)
    hn, hp = np.asarray(hit["nrm"], np.float64), np.asarray(hit["pt"], np.float64)
    miss = hit["t"] < np.float32(0)
    mat = np.where(miss, 0, hit["mat"])
    mc32 = mats["color"][mat]                      # [n, 3] float32
    mc = mc32.astype(np.float64).T
    out_c = c64.copy()
    out_c[:, miss] = (c64 * sky64(d64) ** (trace_depth - depth))[:, miss]
    emit = ~miss & (mats["emittance"][mat] > 0)
    out_c[:, emit] = (c64 * mc * mats["emittance"][mat].astype(np.float64))[:, emit]
    live = ~miss & ~emit
    rng = MinStd(seed(it, depth, pixel))
    killed = np.zeros(n, bool)
    if depth > 3:
        q = np.maximum(mc32[:, 0], np.maximum(mc32[:, 1], mc32[:, 2]))
        u = rng.draw(live)
        killed = live & (u > q)
        live = live & ~killed
        out_c[:, live] = (c64 / q.astype(np.float64))[:, live]
    refl = mats["reflective"][mat]
    rough32 = (np.float32(1.0) - mats["refractive"][mat]).astype(np.float32)
    may = live & (refl > 0)
    u = rng.draw(may)
    spec = may & (u < refl)
    kind = np.where(live, np.where(spec, 1, 2), 0)
    out_c[:, live] = (out_c * np.where(spec, mats["spec"][mat].astype(np.float64).T, mc))[:, live]
    r1, r2, r3 = rng.draw(live), rng.draw(live), rng.draw(live)  # diffuse uses two; the engine dies here
    r1d, r2d, r3d = (r.astype(np.float64) for r in (r1, r2, r3))
    rough = rough32.astype(np.float64)
    f = np.where(spec, d64 - 2.0 * (d64 * hn).sum(axis=0) * hn, hn)
    ct = np.sqrt(1.0 - r1d)
    st = np.sqrt(np.maximum(1.0 - ct * ct, 0.0))
    ang = rough * r1d * (np.pi / 2)
    sx = np.where(spec, np.sin(ang), st)
    cx = np.where(spec, np.cos(ang), ct)
    az2 = np.where(spec, r3d, r2d)
    x, y, z = sx * np.cos(2 * np.pi * r2d), cx, sx * np.sin(2 * np.pi * az2)
    t, b, margin = frame(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        pert = _norm(t * x + f * y + b * z)
        sigma = np.where(spec, U24, U24 * (1.0 + ct / st))
    perturbed = ~spec | (rough32 > 0)
    direction = np.where(perturbed, pert, f)
    return dict(miss=miss, kind=kind, alive=(kind > 0) & (depth + 1 < trace_depth), color=out_c, origin=hp + F001 * hn, dir=direction,
                sigma=sigma, sx=sx, perturbed=perturbed, frame_margin=np.where(spec & perturbed, margin, np.inf), r=(r1, r2, r3))


def synthetic_records(n: int = 50000, n_mats: int = 5, seed_: int = 11) -> dict:
    """The synthetic hit records of tests/test_gpu_stages.py test_shade_specular_and_roulette_branches (same generator, same
    order of draws): random unit normals and directions, materials 0 .. n_mats - 1, pixels of a 1080p frame, iterations 1 .. 5000."""
    rng = np.random.default_rng(seed_)
    nrm = rng.normal(size=(3, n)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=0, keepdims=True).astype(np.float32)
    hit = dict(t=rng.uniform(0.1, 10, n).astype(np.float32), nrm=nrm, mat=rng.integers(0, n_mats, n).astype(np.int32),
               pt=rng.uniform(-5, 5, (3, n)).astype(np.float32))
    d = rng.normal(size=(3, n)).astype(np.float32)
    d /= np.linalg.norm(d, axis=0, keepdims=True).astype(np.float32)
    o = rng.uniform(-5, 5, (3, n)).astype(np.float32)
    color = rng.uniform(0.1, 1, (3, n)).astype(np.float32)
    pixel = rng.integers(0, 1920 * 1080, n).astype(np.int32)
    it = rng.integers(1, 5001, n).astype(np.int32)
    return dict(hit=hit, o=o, d=d, color=color, pixel=pixel, it=it)


def take(rec: dict, idx) -> dict:
    """The records idx of a set, contiguous."""
    c = np.ascontiguousarray
    h = rec["hit"]
    return dict(hit=dict(t=c(h["t"][idx]), nrm=c(h["nrm"][:, idx]), mat=c(h["mat"][idx]), pt=c(h["pt"][:, idx])),
                o=c(rec["o"][:, idx]), d=c(rec["d"][:, idx]), color=c(rec["color"][:, idx]), pixel=c(rec["pixel"][idx]), it=c(rec["it"][idx]))


def wave_ordered(kind: np.ndarray, n: int) -> np.ndarray:
    """Indices into a record set (kind per record: 1 specular, 2 diffuse) such that the waves of 64 consecutive elements are, in turn:
    all diffuse, all specular, diffuse with one specular lane at lane 0, the same at lane 63, mixed as drawn — repeated until n
    elements are placed (a ragged last wave where 64 does not divide n).  Records are reused once a kind runs out."""
    spec, diff = np.flatnonzero(kind == 1), np.flatnonzero(kind == 2)
    anyk = np.flatnonzero(kind > 0)
    assert len(spec) and len(diff)
    ns = nd = na = 0
    out = []
    pattern = 0
    while len(out) < n:
        wave = []
        for lane in range(64):
            want_spec = (pattern == 1) or (pattern == 2 and lane == 0) or (pattern == 3 and lane == 63)
            if pattern == 4:
                wave.append(anyk[na % len(anyk)])
                na += 1
            elif want_spec:
                wave.append(spec[ns % len(spec)])
                ns += 1
            else:
                wave.append(diff[nd % len(diff)])
                nd += 1
        out.extend(wave)
        pattern = (pattern + 1) % 5
    return np.array(out[:n], np.int64)
