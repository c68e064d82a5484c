"""shadeAndExtendRays per sample in every arithmetic mode against float64 (tests/shade_ref64.py), through pt_stage_shade, which
launches the mode's own kernel code (shade_decide, bounce_axis, bounce_sample / bounce_sample_float<HW>).

The image tests (tests/test_gpu_arith.py, the fma / fast cases of tests/test_gpu_ref_kernels.py) see a direction or hit-point error
only where it changes which object the next ray hits; here every sample is held on its own:
  decisions exactly — who survives (== the oracle);
  colours — a hit's: the oracle's bits (exact, fma; fast at depth <= 3: products only), within 2 ulp in fast at depth > 3 (the 1-ulp
    v_rcp_f32 and two roundings); a miss's: within 4 (D - depth) 2^-24 relative of c sky64^(D - depth) (three roundings a factor);
  the origin within 1 ulp of max(|hp_k|, 1e-3) per component;  | |dir| - |dir64| | <= 4 * 2^-24 (|dir64| = 1 wherever a direction is
    sampled; a perfect mirror's reflected direction has the length its inputs give it);
  the direction's angle to float64 in units of sigma = 2^-24 (1 + ct / st) (diffuse; the sampling is ill-conditioned as r1 -> 0) or
    2^-24 (specular): at most 4 x the ORACLE's own maximum in those units, measured on the CPU and pinned in shade_ref64.py (4: the
    1.6-ulp float polynomials against libm's <= 1 ulp, a phase that is never rounded, contraction only removing roundings).  fast
    adds the hardware's trig term: sigma_fast = sigma + 2 sX tau_hw, tau_hw measured in isolation by
    tests/test_gpu_fast_math_blocks.py — a wrong draw, factor of revolutions or lane's operand is orders of magnitude outside.
`exact` goes first and equals the oracle bit for bit, which anchors the inputs and the float64 restatement on the device.

Waves: the stage puts element i into lane i % 64 of wave i / 64, and the inputs are ordered (shade_ref64.wave_ordered) so that a wave
is in turn all diffuse, all specular, diffuse with one specular lane at lane 0, the same at lane 63, mixed, and ragged at the end —
the fma mode's specular evaluations sit behind a wave-uniform ballot."""
import numpy as np
import pytest

import ref_kernel_golden as rk
import shade_ref64 as s64

pytestmark = pytest.mark.gpu
MODES = ("exact", "fma", "fast")
TRACE_DEPTH = 8
FACTOR = 4.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulp_distance(a, b):
    ia, ib = (np.ascontiguousarray(x).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.fixture(scope="module")
def cornell(tmp_path_factory):
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    return scenes.write_scene(scenes.cornell_scene_text(), str(tmp_path_factory.mktemp("shade_modes") / "cornell.txt"))


@pytest.fixture()
def renderer():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    made = []

    def make(path, depth, arith):
        for r in made:
            r.free()
        del made[:]
        sc = capi.Scene(path, res=(64, 64))
        sc.trace_depth = depth
        made.append(capi.Renderer(sc, arith=arith))
        return made[0]
    yield make
    for r in made:
        r.free()


def check(arith, what, rec, depth, trace_depth, got, orc, mats, stats):
    """One stage call against the oracle's call (PORTABLE) and float64; folds the measured ratios into `stats`."""
    go, gd, gc, galive = got
    oo, od, oc, orem = orc
    r = s64.shade(mats, trace_depth, depth, rec["it"], rec["pixel"], rec["hit"], rec["d"], rec["color"])
    b, miss = r["kind"] > 0, r["miss"]
    for a in (go, gd, gc):
        assert np.isfinite(a).all(), what
    # decisions
    assert np.array_equal(galive.astype(bool), orem > 0), (what, np.flatnonzero(galive.astype(bool) != (orem > 0))[:8])
    assert np.array_equal(galive.astype(bool), r["alive"]), what
    if arith == "exact":
        assert np.array_equal(bits(go[:, b]), bits(oo[:, b])) and np.array_equal(bits(gd[:, b]), bits(od[:, b])), what
    # colours
    hit = ~miss
    if arith != "fast" or depth <= 3:
        bad = (bits(gc) != bits(oc)).any(axis=0) & hit
        assert not bad.any(), (what, "hit colour bits", np.flatnonzero(bad)[:8])
    else:
        du = ulp_distance(gc, oc)[:, hit]
        stats["colour_ulp"] = max(stats.get("colour_ulp", 0), int(du.max()) if du.size else 0)
        assert du.size == 0 or du.max() <= 2, (what, "hit colour ulp", int(du.max()))
    if miss.any():
        want = r["color"][:, miss]
        rel = np.abs(gc[:, miss].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
        stats["miss_rel"] = max(stats.get("miss_rel", 0.0), float(rel.max() / ((trace_depth - depth) * s64.U24)))
        assert rel.max() <= 4 * (trace_depth - depth) * s64.U24, (what, "miss colour", float(rel.max()))
    if not b.any():
        return
    # the new origin
    hp = rec["hit"]["pt"]
    tol = np.spacing(np.maximum(np.abs(hp), np.float32(1e-3)).astype(np.float32)).astype(np.float64)
    oerr = (np.abs(go.astype(np.float64) - r["origin"]) / tol)[:, b]
    stats["origin_ulp"] = max(stats.get("origin_ulp", 0.0), float(oerr.max()))
    assert oerr.max() <= 1.0, (what, "origin", float(oerr.max()), np.argwhere(oerr > 1.0)[:4].tolist())
    # the new direction
    nerr = np.abs(np.linalg.norm(gd.astype(np.float64), axis=0) - np.linalg.norm(r["dir"], axis=0))[b]
    stats["norm"] = max(stats.get("norm", 0.0), float(nerr.max() / s64.U24))
    assert nerr.max() <= 4 * s64.U24, (what, "|dir|", float(nerr.max()))
    sigma = r["sigma"] + (2.0 * np.abs(r["sx"]) * s64.TAU_HW if arith == "fast" else 0.0)
    ratio = s64.angle(gd, r["dir"]) / sigma
    keep = b & (r["frame_margin"] >= s64.FRAME_MARGIN)
    stats["bounced"] = stats.get("bounced", 0) + int(b.sum())
    stats["left_out"] = stats.get("left_out", 0) + int((b & ~keep).sum())
    for name, sel, yard in (("diffuse", keep & (r["kind"] == 2), s64.ORACLE_DIFFUSE_MAX), ("specular", keep & (r["kind"] == 1), s64.ORACLE_SPECULAR_MAX)):
        if sel.any():
            worst = int(np.flatnonzero(sel)[np.argmax(ratio[sel])])
            stats[name] = max(stats.get(name, 0.0), float(ratio[worst]))
            assert ratio[worst] <= FACTOR * yard, (what, name, float(ratio[worst]), f"sample {worst}: r = {[float(x[worst]) for x in r['r']]}, "
                                                   f"got {gd[:, worst].tolist()}, float64 {r['dir'][:, worst].tolist()}")


def run(R, oracle, rec, depth, trace_depth):
    got = R.stage_shade(depth, rec["it"], rec["pixel"], rec["hit"], rec["o"], rec["d"], rec["color"])
    orc = oracle.shade(depth, rec["it"], rec["pixel"], rec["hit"], rec["o"], rec["d"], rec["color"], np.full(len(rec["it"]), trace_depth - depth, np.int32))
    return got, orc


@pytest.mark.parametrize("arith", MODES)
def test_synthetic_samples_per_mode(renderer, oracle, cornell, arith):
    """cornell's materials (diffuse, emitter, the rough mirror — roughness 1) at depths 0, 3, 4, 6 (roulette from 4 on): n = 1, 63,
    64, 65 in wave order, the 50,000 records as drawn at each depth, and one run of 200,000 in wave order."""
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.load_scene(cornell)
    mats = s64.materials(oracle.materials())
    R = renderer(cornell, TRACE_DEPTH, arith)
    base = s64.synthetic_records()
    stats = {}
    try:
        for depth in (0, 3, 4, 6):
            kind = s64.shade(mats, TRACE_DEPTH, depth, base["it"], base["pixel"], base["hit"], base["d"], base["color"])["kind"]
            sets = [(f"n={n}", s64.take(base, s64.wave_ordered(kind, n))) for n in (1, 63, 64, 65)] + [("as drawn", base)]
            if depth in (0, 4):
                sets.append(("200000 in wave order", s64.take(base, s64.wave_ordered(kind, 200000))))
            for label, rec in sets:
                got, orc = run(R, oracle, rec, depth, TRACE_DEPTH)
                check(arith, f"{arith} depth {depth} {label}", rec, depth, TRACE_DEPTH, got, orc, mats, stats)
    finally:  # the figures, whatever the assertions say
        print(f"SHADE {arith} synthetic: angle / sigma max diffuse {stats.get('diffuse', 0):.2f} (bound {FACTOR * s64.ORACLE_DIFFUSE_MAX:.1f}), "
              f"specular {stats.get('specular', 0):.2f} (bound {FACTOR * s64.ORACLE_SPECULAR_MAX:.1f}); {stats}")
    assert stats["left_out"] <= s64.FRAME_LEFT_OUT_CAP * stats["bounced"] and stats["diffuse"] > 0 and stats["specular"] > 0


@pytest.mark.parametrize("arith", MODES)
def test_golden_branch_vectors_per_mode(renderer, oracle, arith):
    """The vectors of tests/golden/ref_kernels.bin.gz on ref_shade.txt, built to take every branch: pure mirror, rough mirror,
    partly reflective, emitter, both roulette outcomes, depth 63, axis-aligned and negative-zero normals."""
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.load_scene(rk.SHADE_SCENE)
    mats = s64.materials(oracle.materials())
    v = rk.shade_vectors()
    live_in = v["remaining"] > 0
    stats, seen = {}, 0
    try:
        for depth, remaining in sorted({(int(d), int(r)) for d, r in zip(v["depth"][live_in], v["remaining"][live_in])}):
            sel = np.flatnonzero(live_in & (v["depth"] == depth) & (v["remaining"] == remaining))
            seen += len(sel)
            rec = dict(hit=rk.hit_of(v, sel), o=rk.soa(v["o"][sel]), d=rk.soa(v["d"][sel]), color=rk.soa(v["color"][sel]),
                       pixel=np.ascontiguousarray(v["idx"][sel]), it=np.ascontiguousarray(v["iter"][sel]))
            R = renderer(rk.SHADE_SCENE, depth + remaining, arith)
            got, orc = run(R, oracle, rec, depth, depth + remaining)
            # the oracle's single call applies the sky factor once; float64 carries the miss colours, so only the hits are compared with it
            check(arith, f"{arith} golden depth {depth} remaining {remaining}", rec, depth, depth + remaining, got, orc, mats, stats)
    finally:
        print(f"SHADE {arith} golden: angle / sigma max diffuse {stats.get('diffuse', 0):.2f}, specular {stats.get('specular', 0):.2f}; {stats}")
    assert seen == live_in.sum() > 2000
