"""Grid walk == BVH scan, per ray, bit for bit, in every arithmetic mode ("a leaf is a candidate exactly when
the ray passes its own box test, so any structure that finds a superset of those leaves gives the same image").

The fused kernels of large scenes find their candidates with the uniform-grid walk (csrc/pt_grid.inc); pt_stage_intersect_grid runs
that walk — the same grid_search / grid_filter / walk_start — on caller-supplied rays, in the depth-0 form (k_primary's: the
reference's arithmetic on the reference's boxes in every mode) and in the bounce form (k_paths': the mode's arithmetic).  The scan
side is pt_stage_intersect of a renderer that walks no grid (debug_flags 512); for the depth-0 form of the fma / fast builds it is the
exact-mode renderer.  Rays: grid_rays.py, built against the grid the renderer actually walks (Renderer.grid_info), about 70 k per
scene and box variant (with the traversal boxes of a large scene / with the reference's boxes, debug_flags 2048).  No tolerance and
no ray left out: t, mat, nrm and pt are equal bit for bit on every ray; in exact mode both sides also equal the oracle (PORTABLE),
which anchors the rays before they judge the other modes.

Origins outside the scene bounds (the `outside` family) run where no sphere leaf is tightened (PtStats.tight_leaves == 0: with the
reference's boxes, and on scenes without spheres): tightened boxes are sized for origins inside the bounds and pt_stage_intersect
refuses others, so there is no scan side for them.

Measured on an MI355X: 0.04 - 0.1 s per case (both box variants, about 145 k rays), 0.3 - 1.2 s for the first case of a scene, which
builds its rays and the oracle's answers; the whole module 8 s."""
import time

import numpy as np
import pytest

import grazing_rays as gr
import grid_rays
from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes

pytestmark = pytest.mark.gpu
FIELDS = ("t", "mat", "nrm", "pt")
VARIANTS = {"traversal boxes": dict(flags=0, tail=63, seed=3), "reference boxes": dict(flags=2048, tail=1, seed=4)}
RAYS = 70000


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    """Per scene and box variant, built once and left unchanged: the scene, the walked grid, the rays, the oracle's hits; and the
    scan side's records per arithmetic mode, which the two forms share."""
    from oracle import binding as ob
    made = {}

    def get(name, variant):
        key = (name, variant)
        if key not in made:
            V = VARIANTS[variant]
            path = scenes.write_scene(grid_rays.scene_text(name), str(tmp_path_factory.mktemp(name) / f"{name}.txt"))
            sc = capi.Scene(path)
            r = capi.Renderer(sc, debug_flags=256 | V["flags"])
            try:
                st = r.stats()
                info, longest = r.grid_info()
            finally:
                r.free()
            assert st.grid_cells == info.num_cells == info.res[0] * info.res[1] * info.res[2] and info.num_leaves == sc.desc.num_geoms
            boxes, root = grid_rays.leaf_boxes_of(sc, V["flags"] != 0)
            assert (st.tight_leaves > 0) == (sc.traversal_boxes()[1] > 0 and not V["flags"])
            rays = grid_rays.rays(info, boxes, root, total=RAYS, seed=V["seed"], outside=st.tight_leaves == 0, tail=V["tail"])
            ob.set_math_mode(ob.PORTABLE)
            ob.load_scene(path)
            ref = ob.intersect(rays["o"], rays["d"])
            ob.set_math_mode(ob.LIBM)
            made[key] = dict(scene=sc, path=path, flags=V["flags"], info=info, grid=grid_rays.Grid(info), longest=longest, tight=st.tight_leaves, rays=rays,
                             oracle=ref, scan={})
        return made[key]
    return get


def scan_side(P, arith, legacy=False):
    key = (arith, legacy)
    if key not in P["scan"]:
        r = capi.Renderer(P["scene"], debug_flags=512 | P["flags"], arith=arith, legacy_traversal=legacy)
        try:
            assert r.stats().grid_cells == 0 and r.stats().tight_leaves == P["tight"]
            P["scan"][key] = r.stage_intersect(P["rays"]["o"], P["rays"]["d"])
        finally:
            r.free()
    return P["scan"][key]


def grid_side(P, arith, primary):
    r = capi.Renderer(P["scene"], debug_flags=256 | P["flags"], arith=arith)
    try:
        info, longest = r.grid_info()
        assert r.stats().grid_cells > 0 and r.stats().tight_leaves == P["tight"]
        assert (list(info.res), list(info.origin), list(info.cell_size), info.pad, longest) == \
               (list(P["info"].res), list(P["info"].origin), list(P["info"].cell_size), P["info"].pad, P["longest"]), "every mode walks the same grid"
        return r.stage_intersect_grid(P["rays"]["o"], P["rays"]["d"], primary)
    finally:
        r.free()


def differing(a, b):
    """Per field, the rays whose values differ bit for bit."""
    as_bits = lambda v: gr.bits(v.view(np.float32) if v.dtype == np.int32 else v)
    return {k: (as_bits(a[k]) != as_bits(b[k])).reshape(-1, a["t"].size).any(axis=0) for k in FIELDS}


def report(what, bad, P, a, b, names):
    rows = [f"{what}: {int(bad.sum())} of {bad.size} rays differ; by family: "
            + ", ".join(f"{f} {int(bad[P['rays']['family'] == i].sum())}" for i, f in enumerate(grid_rays.FAMILIES))]
    for i in np.flatnonzero(bad)[:8]:
        rows.append("  " + grid_rays.describe(P["rays"], i, P["grid"]))
        rows.append(f"    {names[0]}: " + ", ".join(f"{k}={a[k][..., i].tolist()}" for k in FIELDS))
        rows.append(f"    {names[1]}: " + ", ".join(f"{k}={b[k][..., i].tolist()}" for k in FIELDS))
    return "\n".join(rows)


def all_equal(what, P, a, b, names):
    bad = differing(a, b)
    for k in FIELDS:
        assert not bad[k].any(), report(f"{what}, {k}", bad[k], P, a, b, names)


def the_comparison_means_something(name, P):
    """Conditions on the scene and its rays, from the oracle's answers alone (tests/test_grid_rays_host.py checks the same on the
    grid of pt_build_grid without a GPU)."""
    R, H, G = P["rays"], P["oracle"], P["grid"]
    fam = lambda f: R["family"] == grid_rays.FAMILIES.index(f)
    aimed = fam("leaf") | fam("lattice")
    cluster = grid_rays.in_cluster(name, H)
    far = grid_rays.travel(G, R, H["t"])[fam("long")] > 0.5 * G.diagonal
    assert cluster[aimed].mean() >= 0.25 and (~cluster[aimed]).mean() >= 0.25, cluster[aimed].mean()
    assert far.mean() >= 0.5, far.mean()
    if name == "crowded":  # more records in one cell than a lane files in a turn (63) and than a step files at once (192)
        assert P["longest"] > 192, P["longest"]
    return cluster[aimed].mean(), far.mean()


@pytest.mark.parametrize("form", ["primary", "bounce"])
@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
@pytest.mark.parametrize("name", list(grid_rays.SCENES))
def test_grid_walk_reports_what_the_scan_reports(prepared, name, arith, form):
    primary = form == "primary"
    t0 = time.time()
    for variant in VARIANTS:
        P = prepared(name, variant)
        R = P["rays"]
        n = R["o"].shape[1]
        assert n <= 80000 and n % 64 == VARIANTS[variant]["tail"]
        share, far = the_comparison_means_something(name, P)
        counts = {f: int((R["family"] == i).sum()) for i, f in enumerate(grid_rays.FAMILIES)}
        assert all(counts[f] > 0 for f in grid_rays.FAMILIES if f != "outside") and (counts["outside"] > 0) == (P["tight"] == 0)
        what = f"{name} ({variant}, grid {list(P['info'].res)}, longest cell list {P['longest']}) {arith} {form} form"
        print(f"{what}: {n} rays {counts}; leaf / lattice rays ending in the cluster {share:.3f}, long rays beyond half the diagonal {far:.3f}")
        # the depth-0 form is traced in the reference's arithmetic in every mode: its scan side is the exact-mode renderer
        scan = scan_side(P, "exact" if primary else arith)
        grid = grid_side(P, arith, primary)
        for side, hit in (("scan", scan), ("grid walk", grid)):
            for k in ("t", "nrm", "pt"):
                assert np.isfinite(hit[k]).all(), f"{what}, {side} {k}: {int((~np.isfinite(hit[k])).sum())} values are not finite"
        if arith == "exact":  # anchors the rays to the oracle before they judge the other modes
            all_equal(f"{what}: scan against the oracle", P, scan, P["oracle"], ("scan", "oracle"))
            all_equal(f"{what}: grid walk against the oracle", P, grid, P["oracle"], ("grid walk", "oracle"))
        all_equal(f"{what}: grid walk against the scan", P, grid, scan, ("grid walk", "scan"))
        if arith == "exact" and not primary:  # once per scene: the per-lane walk from the root as a third scan side
            all_equal(f"{what}: grid walk against the per-lane walk", P, grid, scan_side(P, arith, legacy=True), ("grid walk", "per-lane walk"))
        if P["tight"] == 0:  # rays parallel to an outer face, just outside it: nothing there
            beside = (R["family"] == grid_rays.FAMILIES.index("outside")) & (R["feature"] == len(grid_rays.OUTSIDE_KINDS) - 1)
            assert beside.sum() > 100 and (grid["t"][beside] == -1.0).all() and (P["oracle"]["t"][beside] == -1.0).all()
    print(f"{name} {arith} {form}: {time.time() - t0:.2f} s")


# Found by the comparison above (mixed_sizes, plane family): rays in a symmetry plane of the scene-sized sphere that start inside it.
# The reference negates the finished normal of a hit seen from inside, so the component that is zero by symmetry comes out as -0.0; the
# grid's lean chunks negated the object-space normal before the matrix product instead, where terms that cancel give +0.0 either way.
INSIDE_SPHERE = np.array([  # origin, direction
    [5.589927673339844, 1.8913594484329224, 0.0, -0.6522392630577087, -0.7580131888389587, 0.0],
    [0.9844179153442383, -4.485680103302002, 0.0, -0.9976659417152405, 0.06828374415636063, 0.0],
    [0.0, 0.7084755897521973, -2.6788384914398193, 0.0, 0.0, 1.0],
    [-0.5369898676872253, -0.7489624619483948, 1.401298464324817e-45, 0.5422549247741699, 0.8402140140533447, -0.0],
], np.float32)


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_regression_normal_of_a_sphere_seen_from_inside_keeps_its_negative_zero(prepared, arith):
    P = dict(prepared("mixed_sizes", "traversal boxes"))
    o, d = np.ascontiguousarray(INSIDE_SPHERE[:, :3].T), np.ascontiguousarray(INSIDE_SPHERE[:, 3:].T)
    from oracle import binding as ob
    ob.set_math_mode(ob.PORTABLE)
    ob.load_scene(P["path"])
    ref = ob.intersect(o, d)
    ob.set_math_mode(ob.LIBM)
    assert (ref["geom"] == 1).all() and ((ref["nrm"] == 0) & np.signbit(ref["nrm"])).any(axis=0).all()  # the sphere, and a -0.0 in every normal
    n = o.shape[1]
    P.update(rays=dict(o=o, d=d, family=np.full(n, grid_rays.FAMILIES.index("uniform"), np.int8), feature=np.full(n, -1), delta=np.zeros(n), leaf=np.full(n, -1)), scan={})
    for primary in (True, False):
        grid, scan = grid_side(P, arith, primary), scan_side(P, "exact" if primary else arith)
        all_equal(f"rays inside the sphere, {arith}, {'primary' if primary else 'bounce'} form: grid walk against the scan", P, grid, scan, ("grid walk", "scan"))
        if arith == "exact":
            all_equal(f"rays inside the sphere, {'primary' if primary else 'bounce'} form: grid walk against the oracle", P, grid, ref, ("grid walk", "oracle"))


def test_refusals(prepared):
    """On the host, by name and phrase (tests/test_gpu_refusals.py): no grid, null pointers, the origin rule of tightened leaves."""
    P = prepared("mixed_sizes", "traversal boxes")
    o, d = np.ascontiguousarray(P["rays"]["o"][:, :64]), np.ascontiguousarray(P["rays"]["d"][:, :64])
    lib = capi.lib()

    def refused(who, phrase, call, *args):
        with pytest.raises(capi.PtError) as e:
            call(*args)
        assert str(e.value).startswith(who + ": ") and phrase in str(e.value), str(e.value)

    r = capi.Renderer(P["scene"], debug_flags=512)
    try:
        refused("pt_stage_intersect_grid", "walks no grid", r.stage_intersect_grid, o, d)
        refused("pt_stage_grid_info", "walks no grid", r.grid_info)
    finally:
        r.free()
    r = capi.Renderer(P["scene"], debug_flags=256)
    try:
        assert r.stats().tight_leaves > 0
        out = r.stage_intersect_grid(o, d)
        assert lib.pt_stage_intersect_grid(0, None, None, 0, None, None, None, None) == 0  # n <= 0: nothing to do
        f, i = capi._f, capi._i
        assert lib.pt_stage_intersect_grid(64, f(o), f(d), 0, f(out["t"]), None, i(out["mat"]), f(out["pt"])) == -1
        assert lib.pt_last_error().decode().startswith("pt_stage_intersect_grid: null argument")
        assert lib.pt_stage_grid_info(None, None) == -1 and lib.pt_last_error().decode().startswith("pt_stage_grid_info: null argument")
        far = o.copy()
        far[0, 5] = np.float32(1e3)  # outside the bounds: fine for the depth-0 form, refused for the bounce form (as pt_stage_intersect does)
        assert np.isfinite(r.stage_intersect_grid(far, d, True)["t"]).all()
        refused("pt_stage_intersect_grid", "ray 5 starts outside the scene bounds", r.stage_intersect_grid, far, d, False)
        refused("pt_stage_intersect", "ray 5 starts outside the scene bounds", r.stage_intersect, far, d)
    finally:
        r.free()
