"""Hierarchical search == flat leaf tests, per ray, in every arithmetic mode (DESIGN.md sections 4, 5, 9: "the structure never
changes which leaves pass their own box test").  No float64 comparison and no tolerance: each mode is compared WITH ITSELF,
bit for bit, on rays built to graze the leaf boxes (grazing_rays.py).

Hierarchical side: the whole scene (top list plus subtree scans, or the per-lane walk from the root with legacy_traversal)
through pt_stage_intersect, which runs the mode's own bounce arithmetic — in the fast build the centre / half-extent boxes
with the slack of the inner ones (csrc/pt_tables.cpp center_half_box).  debug_flags 2048 keeps the reference's leaf boxes (both
sides test the same leaf boxes), 512 forbids the grid.
Flat side: the same primitives in sub-scenes of the six walls plus at most 26 cluster primitives, <= 32 leaves, so every leaf
is a top entry tested directly and no inner box is involved; a ray's flat result is the sub-scene result with the smallest
t >= 0 (first sub-scene on ties), a miss if all miss.
A tie between two primitives is resolved by visiting order, which the two sides do not share: where the sub-scenes that attain
the minimum disagree about mat / nrm / pt the ray is left out of that comparison (at most 0.1 % of the rays may be); a tie
INSIDE one sub-scene cannot be seen from outside, so the scenes have no coincident faces (grazing_rays.objects), and in exact
mode the oracle, the hierarchical and the flat side agree in every field on every ray.

Triangles (the `mesh` extension) have the leaf boxes least like the others: padded by 1e-4 max(1, |coord|) because a flat box never
passes the strict slab test, left alone by the tight-leaf pass, wrapped by the fast build's inner boxes, and carried by their own `tri`
flag through the search kernels.  The tri_* scenes put 96 / 400 triangles (closed octahedra, axis-aligned quads), each its own leaf,
where the cubes and spheres were; the rays graze the padded boxes and, in two more families, aim at the triangles' own edges and
vertices.  Triangles that share an edge DO tie there, so the flat side deals them out to different sub-scenes, where the tie is seen
(grazing_rays.flat_scene_texts), and the tri_edge / tri_vertex families, a good part of which ties, take part in the comparison of t
on every ray and, in exact mode, of every field with the oracle, but not in the comparison of mat / nrm / pt between the two sides."""
import numpy as np
import pytest

import grazing_rays as gr
from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes

pytestmark = pytest.mark.gpu
FLAGS = 2048 | 512
FIELDS = ("t", "mat", "nrm", "pt")
TRI_RAYS = {"tri_room": 120000, "tri_hall": 120000, "tri_big": 100000}  # asked for; every feature x delta at least once gives 121 k, 121 k, 150 k


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    """Per scene, built once and left unchanged: the scene and its flat sub-scenes, the leaf boxes, the rays, the oracle's hits."""
    from oracle import binding as ob
    made = {}

    def get(name):
        if name not in made:
            d = tmp_path_factory.mktemp(name)
            path = scenes.write_scene(gr.scene_text(name), str(d / f"{name}.txt"))
            sc = capi.Scene(path)
            boxes, leaf_of, _ = gr.tree(sc.bvh())
            flat = [capi.Scene(scenes.write_scene(text, str(d / f"{name}_{k}.txt"))) for k, text in enumerate(gr.flat_scene_texts(name))]
            assert all(f.desc.num_geoms <= 32 for f in flat) and sum(f.desc.num_geoms - gr.WALLS for f in flat) == sc.desc.num_geoms - gr.WALLS
            if name.startswith("tri_"):
                rays = gr.rays(boxes[leaf_of], boxes[0], total=TRI_RAYS[name], families=gr.FAMILIES, tris=gr.triangles(sc.geoms()), limit=150000)
            else:
                rays = gr.rays(boxes[leaf_of], boxes[0])
            ob.set_math_mode(ob.PORTABLE)
            ob.load_scene(path)
            ref = ob.intersect(rays["o"], rays["d"])
            ob.set_math_mode(ob.LIBM)
            made[name] = dict(scene=sc, flat=flat, leaf_boxes=boxes[leaf_of], nodes=len(boxes), rays=rays, oracle=ref)
        return made[name]
    return get


def intersect(scene, o, d, flags=FLAGS, **kw):
    r = capi.Renderer(scene, debug_flags=flags, **kw)
    try:
        # (without bit 2048 the tight-leaf pass runs on scenes of 64 nodes and more: it tightens sphere leaves only, and the tri_* scenes,
        # the only ones searched without the bit, have none — a triangle's padded box must stay as it is)
        assert r.stats().grid_cells == 0 and r.stats().tight_leaves == 0
        return r.stage_intersect(o, d)
    finally:
        r.free()


def differing(a, b):
    """Per field, the rays whose values differ bit for bit."""
    return {k: (gr.bits(a[k].view(np.float32) if k == "mat" else a[k]) != gr.bits(b[k].view(np.float32) if k == "mat" else b[k])).reshape(-1, a["t"].size).any(axis=0)
            for k in FIELDS}


def report(what, bad, P, a, b):
    rows = [f"{what}: {int(bad.sum())} of {bad.size} rays differ"]
    for i in np.flatnonzero(bad)[:8]:
        rows.append("  " + gr.describe(P["rays"], i, P["leaf_boxes"]))
        rows.append("    one:   " + ", ".join(f"{k}={a[k][..., i].tolist()}" for k in FIELDS))
        rows.append("    other: " + ", ".join(f"{k}={b[k][..., i].tolist()}" for k in FIELDS))
    return "\n".join(rows)


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
@pytest.mark.parametrize("name", ["room", "hall", "big"])
def test_hierarchical_search_reports_what_flat_leaf_tests_report(prepared, name, arith):
    P = prepared(name)
    o, d = P["rays"]["o"], P["rays"]["d"]
    n = o.shape[1]
    assert P["nodes"] == {"room": 191, "hall": 191, "big": 811}[name] and 280000 <= n <= 320000
    flat, agree = gr.combine_flat([intersect(f, o, d, arith=arith) for f in P["flat"]])
    for k in ("t", "nrm", "pt"):
        assert np.isfinite(flat[k]).all(), f"flat {k}: {int((~np.isfinite(flat[k])).sum())} values are not finite"
    # the comparison must mean something: the grazing rays are decided both ways, the clear hits see the cluster
    grazing = P["rays"]["family"] <= gr.FAMILIES.index("corner")
    cluster = gr.reports_cluster(name, flat)
    print(f"{name} {arith}: {n} rays, grazing rays reporting the cluster {cluster[grazing].mean():.3f}, left out of the mat / nrm / pt comparison {int((~agree).sum())}")
    assert cluster[grazing].mean() >= 0.25 and (~cluster[grazing]).mean() >= 0.25
    assert cluster[P["rays"]["family"] == gr.FAMILIES.index("face")].mean() >= 0.5
    assert (~agree).sum() <= 0.001 * n  # a condition on the scene and rays, not a measurement of the kernels
    for legacy in (False, True):
        hier = intersect(P["scene"], o, d, arith=arith, legacy_traversal=legacy)
        what = f"{name} {arith} {'per-lane walk from the root' if legacy else 'top list + subtree scans'}"
        for k in ("t", "nrm", "pt"):
            assert np.isfinite(hier[k]).all(), f"{what} {k}: {int((~np.isfinite(hier[k])).sum())} values are not finite"
        if arith == "exact":  # anchors the rays and the flat combination to the oracle before they judge the other modes
            bad = differing(hier, P["oracle"])
            for k in FIELDS:
                assert not bad[k].any(), report(f"{what} against the oracle, {k}", bad[k], P, hier, P["oracle"])
        bad = differing(hier, flat)
        assert not bad["t"].any(), report(f"{what} against flat leaf tests, t", bad["t"], P, hier, flat)
        for k in ("mat", "nrm", "pt"):
            assert not (bad[k] & agree).any(), report(f"{what} against flat leaf tests, {k}", bad[k] & agree, P, hier, flat)


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
@pytest.mark.parametrize("name,flags", [("tri_room", FLAGS), ("tri_hall", FLAGS), ("tri_big", FLAGS), ("tri_big", 512)],
                         ids=["tri_room", "tri_hall", "tri_big", "tri_big default tables"])
def test_triangle_leaves_hierarchical_search_reports_what_flat_leaf_tests_report(prepared, name, flags, arith):
    """The same comparison on the triangle scenes.  flags 512 alone: the default tables, where the tight-leaf pass has run (811 nodes)
    and must have left every triangle's box alone (`intersect` asserts tight_leaves == 0: the scene has no sphere)."""
    P = prepared(name)
    o, d = P["rays"]["o"], P["rays"]["d"]
    n = o.shape[1]
    fam = P["rays"]["family"]
    assert P["nodes"] == {"tri_room": 203, "tri_hall": 203, "tri_big": 811}[name] and 100000 <= n <= 150000
    assert all(g.type == 2 for g in P["scene"].geoms()[gr.WALLS:]) and set(np.unique(fam)) == set(range(len(gr.FAMILIES)))
    flat, agree = gr.combine_flat([intersect(f, o, d, flags=flags, arith=arith) for f in P["flat"]])
    for k in ("t", "nrm", "pt"):
        assert np.isfinite(flat[k]).all(), f"flat {k}: {int((~np.isfinite(flat[k])).sum())} values are not finite"
    # conditions on the scene and the rays, checked with the oracle on the CPU before they were fixed (exact mode: 0.30 of the grazing
    # rays and 0.53 of the triangle-aimed ones report the cluster; at most 3 rays of the compared families are left out)
    grazing = fam <= gr.FAMILIES.index("corner")
    aimed = fam >= gr.FAMILIES.index("tri_edge")
    compared = agree & ~aimed
    cluster = gr.reports_cluster(name, flat)
    print(f"{name} {arith}: {n} rays, reporting the cluster: grazing {cluster[grazing].mean():.3f}, aimed at triangles {cluster[aimed].mean():.3f}; "
          f"left out of the mat / nrm / pt comparison beside the aimed ones {int((~agree & ~aimed).sum())}, ties among the aimed ones {int((~agree & aimed).sum())}")
    assert cluster[grazing].mean() >= 0.25 and (~cluster[grazing]).mean() >= 0.25
    assert cluster[aimed].mean() >= 0.25 and (~cluster[aimed]).mean() >= 0.10
    assert (~agree & ~aimed).sum() <= 0.001 * n
    for legacy in (False, True):
        hier = intersect(P["scene"], o, d, flags=flags, arith=arith, legacy_traversal=legacy)
        what = f"{name} {arith} {'per-lane walk from the root' if legacy else 'top list + subtree scans'}"
        for k in ("t", "nrm", "pt"):
            assert np.isfinite(hier[k]).all(), f"{what} {k}: {int((~np.isfinite(hier[k])).sum())} values are not finite"
        if arith == "exact":  # every field, every ray, every family
            bad = differing(hier, P["oracle"])
            for k in FIELDS:
                assert not bad[k].any(), report(f"{what} against the oracle, {k}", bad[k], P, hier, P["oracle"])
        bad = differing(hier, flat)
        assert not bad["t"].any(), report(f"{what} against flat leaf tests, t", bad["t"], P, hier, flat)
        for k in ("mat", "nrm", "pt"):
            assert not (bad[k] & compared).any(), report(f"{what} against flat leaf tests, {k}", bad[k] & compared, P, hier, flat)
