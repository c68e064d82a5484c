"""The dynamic-LDS byte maps of the traversal kernels (csrc/pt_lds.h), without a GPU.

A kernel takes every LDS pointer from its map and the launch code requests the map's `total`, so what can still go wrong is the
map itself.  tests/lds_layout_driver.cpp, built with the system compiler, prints every map for a sweep of scene sizes; here the
regions must be in order and must not overlap, everything accessed 16 bytes at a time must start on a multiple of 16, `total`
must be the end of the last region — and equal the byte counts the launch code requested before the maps existed (the closed
forms of fused_lds_bytes / primary_grid_lds_bytes / paths_lds_bytes and of the intersect / shade launches, restated below), so
that the same scenes still get the same resident workgroups per CU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")


def _fields(tokens):
    return {k: int(v) for k, v in (t.split("=") for t in tokens)}


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds") / "lds_layout_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "lds_layout_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    consts, waves, cases = {}, {}, []
    for line in out.splitlines():
        name, *tokens = line.split()
        if name == "sizes":
            consts = _fields(tokens)
        elif name.startswith("wave."):
            waves[name[5:]] = _fields(tokens)
        elif name == "case":
            cases.append((_fields(tokens), {}))
        else:
            cases[-1][1][name] = _fields(tokens)
    return consts, waves, cases


def _in_order(regions, total, what):
    """regions: (name, offset, bytes the kernel puts there, required alignment) in map order."""
    end = 0
    for name, off, need, align in regions:
        assert off >= end, f"{what}: {name} at {off} overlaps the previous region (ends at {end})"
        assert off % align == 0, f"{what}: {name} at {off} is not {align}-byte aligned"
        assert need >= 0
        end = off + need
    assert total == end, f"{what}: total {total}, last region ends at {end}"


def r16(x):
    return (x + 15) & ~15


# ── the per-wave blocks, restated from the structs they hold ────────────────────────────────────────────────────────────────
K_RING, K_CELL_RING, K_CAND_CAP, K_VISIT_RING = 128, 256, 192, 64
WAVE_LDS = 64 * 8 + 7 * 64 * 4 + K_CAND_CAP * 4
LANES = 64 * 8 + 6 * 64 * 4 + K_RING * 2
SLOTS = 64 * 16 + 64 * 16 + 64 * 4 + 64 * 4 + 64 * 4


def carry_bytes(small, npar):
    return npar * 64 * 8 + npar * 6 * 64 * 4 + K_RING * (2 if small else 4) + npar * (3 if small else 6) * 64 * 4 + (0 if small else 64 * 4)


def rinv_planes(fast, ex):
    return 3 if (ex or not fast) else 6


def grid_wave_bytes(fast, ex):
    return carry_bytes(False, 1) + K_CELL_RING * 4 + K_RING * 4 + rinv_planes(fast, ex) * 64 * 4


def paths_extra_bytes(mode):
    return (SLOTS if mode == 0 else 0) + 64 * 4 + K_VISIT_RING * 4


def paths_wave_bytes(mode, fast):
    return (LANES if mode == 0 else carry_bytes(False, 1) if mode == 1 else grid_wave_bytes(fast, False)) + paths_extra_bytes(mode)


def test_struct_sizes_and_constants(maps):
    c, _, cases = maps
    assert (c["Mat"], c["Node"], c["Geom"], c["TopEntry"]) == (48, 32, 272, 32)
    assert all(c[k] % 16 == 0 for k in ("Mat", "Node", "Geom", "TopEntry"))
    assert (c["kMaxTop"], c["kIterHashMax"], c["kWavesPerBlock"]) == (32, 256, 4)
    assert (c["kCandCap"], c["kRing"], c["kCellRing"], c["kVisitRing"]) == (K_CAND_CAP, K_RING, K_CELL_RING, K_VISIT_RING)
    assert (c["kSlotTail"], c["kSlotVisit"], c["kSlotBytes"]) == (2 * 64 * 16, 2 * 64 * 16 + 2 * 64 * 4, SLOTS)
    # the sweep the checks below rest on
    seen = lambda k: {s[k] for s, _ in cases}
    assert seen("top") == set(range(1, 33)) and {7, 5000} <= seen("geoms") and {1, 1000} <= seen("mats")
    assert {255, 256, 257} <= seen("iters") and {1, 64} <= seen("depth") and seen("scan") == {0, 1} and seen("fast") == {0, 1}


def test_per_wave_blocks(maps):
    _, w, _ = maps
    m = w["WaveMap"]
    _in_order([("best", m["best"], 64 * 8, 16), ("rec", m["rec"], 7 * 64 * 4, 16), ("list", m["list"], K_CAND_CAP * 4, 4)], m["bytes"], "WaveMap")
    assert m["bytes"] == WAVE_LDS and m["bytes"] % 16 == 0
    m = w["LanesMap"]
    _in_order([("best", m["best"], 64 * 8, 16), ("rec", m["rec"], 6 * 64 * 4, 16), ("ent", m["ent"], K_RING * 2, 2)], m["bytes"], "LanesMap")
    assert m["bytes"] == LANES and m["bytes"] % 16 == 0
    for name, small, npar in (("small.2", True, 2), ("full.1", False, 1), ("full.2", False, 2)):
        m = w["CarryMap." + name]
        _in_order([("best", m["best"], npar * 64 * 8, 16), ("rec", m["rec"], npar * 6 * 64 * 4, 16),
                   ("ray", m["ray"], npar * (3 if small else 6) * 64 * 4, 16), ("ent", m["ent"], K_RING * (2 if small else 4), 4),
                   ("slot", m["slot"], 0 if small else 64 * 4, 4)], m["bytes"], "CarryMap." + name)
        assert m["bytes"] == carry_bytes(small, npar) and m["bytes"] % 16 == 0
    for fast in (0, 1):
        for ex in (0, 1):
            m = w[f"GridMap.fast{fast}.ex{ex}"]
            assert m["planes"] == rinv_planes(fast, ex)
            _in_order([("carry", 0, carry_bytes(False, 1), 16), ("cells", m["cells"], K_CELL_RING * 4, 4), ("gix", m["gix"], K_RING * 4, 4),
                       ("rinv", m["rinv"], m["planes"] * 64 * 4, 4)], m["bytes"], "GridMap")
            assert m["bytes"] == grid_wave_bytes(fast, ex) and m["bytes"] % 16 == 0
        for mode, form in enumerate(("lds", "scan", "grid")):
            m = w[f"PathsWaveMap.{form}.fast{fast}"]
            core = paths_wave_bytes(mode, fast) - paths_extra_bytes(mode)
            # the refill slots are the targets of global_load_lds_dwordx4: 16-byte aligned, like the block itself
            _in_order([("search", 0, core, 16), ("slots", m["slots"], SLOTS if mode == 0 else 0, 16), ("died", m["died"], 64 * 4, 4),
                       ("fillc", m["fillc"], K_VISIT_RING * 4, 4)], m["bytes"], "PathsWaveMap." + form)
            assert m["bytes"] == paths_wave_bytes(mode, fast) and m["bytes"] % 16 == 0


# ── the launch code's byte counts before the maps (pt_launch.inc of the parent commit), restated ──────────────────────────────
def iter_hash_entries(s):
    return (s["iters"] + 3) & ~3 if s["iters"] <= 256 else 0


def table_bytes(s):
    return s["nodes"] * 32 + s["geoms"] * 272


def fused_lds_bytes(s, in_lds, wave_lds, primary):
    b = s["top"] * 32 + r16(s["mats"] * 48) + 4 * wave_lds + iter_hash_entries(s) * 4
    if in_lds:
        b += r16(table_bytes(s))
    if primary:
        b += s["top"] * 32 + (r16(s["geoms"] * 12) if in_lds else 0)
    return b


def primary_grid_lds_bytes(s, fast, ex):
    return r16(s["mats"] * 48) + 4 * grid_wave_bytes(fast, ex) + iter_hash_entries(s) * 4


def paths_lds_bytes(s, mode, fast):
    common = r16(s["mats"] * 48) + iter_hash_entries(s) * 4 * max(0, s["depth"] - 1)
    top = s["top"] * 32
    if mode == 0:
        return common + top + s["geoms"] * 272 + 4 * paths_wave_bytes(0, fast) + 32 * 4 + 64 * 4
    if mode == 1:
        return common + top + 4 * paths_wave_bytes(1, fast) + (s["nodes"] * 32 if s["scan"] > 0 else 0)
    return common + 4 * paths_wave_bytes(2, fast)


def test_block_maps(maps):
    _, _, cases = maps
    assert len(cases) > 10000
    for s, m in cases:
        fast = s["fast"]
        ex = fast  # depth 0 of the fast (and fma) build runs the exact arithmetic; the exact build has one arithmetic
        top, mats, nodes, geoms = s["top"] * 32, s["mats"] * 48, s["nodes"] * 32, s["geoms"] * 272
        ihash = iter_hash_entries(s) * 4
        what = lambda name: f"{name} {s}"
        for t in (0, 1):
            L = m[f"legacy.{t}"]
            _in_order([("nodes", L["nodes"], nodes * t, 16), ("geoms", L["geoms"], geoms * t, 16)], L["total"], what("legacy"))
            assert L["total"] == (r16(table_bytes(s)) if t else 0)
            L = m[f"intersect.{t}"]
            _in_order([("top", L["top"], top, 16), ("nodes", L["nodes"], nodes * t, 16), ("geoms", L["geoms"], geoms * t, 16),
                       ("waves", L["waves"], 4 * L["wave_bytes"], 16)], L["total"], what("intersect"))
            assert L["wave_bytes"] == WAVE_LDS
            assert L["total"] == (r16(table_bytes(s)) if t else 0) + 4 * WAVE_LDS + top
        for form, e in (("primary", ex), ("bounce", 0)):  # k_intersect_grid: the waves' grid blocks and nothing else
            L = m["intersect_grid." + form]
            assert L["wave_bytes"] == grid_wave_bytes(fast, e) and L["wave_bytes"] % 16 == 0
            _in_order([("waves", L["waves"], 4 * L["wave_bytes"], 16)], L["total"], what("intersect_grid." + form))
            assert L["total"] == 4 * grid_wave_bytes(fast, e) <= 64 * 1024  # (what a kernel gets without asking)
        for form, in_lds, grid in (("lds", 1, 0), ("scan", 0, 0), ("grid", 0, 1)):
            L = m["primary." + form]
            wave = grid_wave_bytes(fast, ex) if grid else carry_bytes(True, 2) if in_lds else WAVE_LDS
            assert L["wave_bytes"] == wave
            _in_order([("top", L["top"], 0 if grid else top, 16), ("mats", L["mats"], mats, 16), ("nodes", L["nodes"], nodes * in_lds, 16),
                       ("geoms", L["geoms"], geoms * in_lds, 16), ("waves", L["waves"], 4 * wave, 16), ("ihash", L["ihash"], ihash, 4),
                       ("cam_top", L["cam_top"], 0 if grid else top, 16), ("cam_qo", L["cam_qo"], r16(s["geoms"] * 12) * in_lds, 4)],
                      L["total"], what("primary." + form))
            assert L["total"] == (primary_grid_lds_bytes(s, fast, ex) if grid else fused_lds_bytes(s, in_lds, wave, True))
        for mode, form in enumerate(("lds", "scan", "grid")):
            L = m["paths." + form]
            assert L["wave_bytes"] == paths_wave_bytes(mode, fast)
            rows = ihash * max(0, s["depth"] - 1)
            _in_order([("top", L["top"], 0 if mode == 2 else top, 16), ("mats", L["mats"], mats, 16), ("geoms", L["geoms"], geoms if mode == 0 else 0, 16),
                       ("nodes", L["nodes"], nodes if mode == 1 and s["scan"] else 0, 16), ("waves", L["waves"], 4 * L["wave_bytes"], 16),
                       ("tword", L["tword"], 32 * 4 if mode == 0 else 0, 4), ("lmat", L["lmat"], 64 * 4 if mode == 0 else 0, 4),
                       ("ihash", L["ihash"], rows, 4)], L["total"], what("paths." + form))
            assert L["total"] == paths_lds_bytes(s, mode, fast)
        L = m["shade"]
        _in_order([("mats", L["mats"], mats, 16), ("ihash", L["ihash"], ihash, 4)], L["total"], what("shade"))
        assert L["total"] == r16(mats) + ihash
        L = m["shade_stage"]
        _in_order([("mats", L["mats"], mats, 16), ("ihash", L["ihash"], 0, 4)], L["total"], what("shade_stage"))
        assert L["total"] == r16(mats)
