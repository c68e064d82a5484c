"""The retire-once rule of csrc/pt_sched.h without a GPU: the map from a slot of a region to (residue, position inside the
sub-region) that k_collect tells a retiree slot by.  (Which batches store and gather their depth-0 retirees once is a rung of
batch_form: tests/test_sched_form.py.)

k_primary puts the depth-0 retirees of sub-region (q, k, rho) at its front; in a retire_once batch those slots are written and
read in iteration 0 only.  k_collect therefore has to know, for slot i of a region, which sub-region holds it and how far in:
sub_slot must invert sub_offset / sub_chunks for every slot, and `position < retirees(rho)` must then pick exactly the first
retirees(rho) slots of every sub-region and nothing else — never a slot of the gap behind the tile's partial last chunk.
tests/sched_retire_once_driver.cpp, built with the system compiler, prints the header's functions over a sweep of tile sizes
(N % 64 != 0 among them), queue counts, residue counts (more residues than chunks among them) and iteration counts (the map is
per region: K only sizes the buffer the regions sit in); here they are checked by enumeration."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")


def _fields(tokens):
    return {k: int(v) for k, v in (t.split("=") for t in tokens)}


def _ints(line):
    return np.array(line.split(), dtype=np.int64)


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """{case name: [(header fields, [number lines])]} of the driver's output."""
    exe = str(tmp_path_factory.mktemp("sched_retire_once") / "sched_retire_once_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_retire_once_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # the header compiles as plain C++, without warnings
    text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    cases = {}
    for line in text.splitlines():
        if line[:1].isalpha() and "=" in line:
            name, *tokens = line.split()
            cases.setdefault(name, []).append((_fields(tokens), []))
            last = cases[name][-1][1]
        else:
            last.append(line)
    return cases


def _sub_regions(my_nq, wq0):
    """[(first slot, slots)] of the sub-regions rho = 0 .. wq0 - 1: residue rho owns the chunks rho, rho + wq0, ... (pt_sched.h)."""
    quo, rem = divmod(my_nq, wq0)
    return [((rho * quo + min(rho, rem)) * 64, (quo + (1 if rho < rem else 0)) * 64) for rho in range(wq0)]


def test_slot_map_inverts_the_sub_regions(out):
    seen = set()
    for f, (slots, _) in out["slots"]:
        N, Q, wq0, K, q, my_nq = f["N"], f["Q"], f["wq0"], f["K"], f["q"], f["my_nq"]
        seen.add((N % 64 != 0, wq0 > my_nq > 0))
        chunks = (N + 63) // 64
        assert my_nq == ((chunks - q + Q - 1) // Q if q < chunks else 0)
        assert my_nq * 64 <= f["seg_cap"] and f["cap"] == K * f["seg_cap"]  # a region's slots end before the next region begins
        v = _ints(slots).reshape(-1, 2) if slots.strip() else np.zeros((0, 2), dtype=np.int64)
        assert len(v) == my_nq * 64
        want = np.zeros_like(v)
        covered = 0
        for rho, (first, n) in enumerate(_sub_regions(my_nq, wq0)):
            assert first == covered  # the sub-regions tile the region in residue order
            want[first:first + n, 0] = rho
            want[first:first + n, 1] = np.arange(n)
            covered += n
        assert covered == my_nq * 64 and np.array_equal(v, want), f
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_every_slot_is_classified_once_and_the_gap_never_is_a_retiree(out):
    gaps = 0
    for f, (_, line) in out["slots"]:
        wq0, my_nq, g0, g1 = f["wq0"], f["my_nq"], f["g0"], f["g1"]
        n = my_nq * 64
        missing = n - f["my_pixels"]
        assert g1 - g0 == missing and (missing == 0 or 0 < missing < 64)
        v = _ints(line).reshape(4, wq0 + n)
        regions = _sub_regions(my_nq, wq0)
        for fill in range(4):
            counts, is_retiree = v[fill, :wq0], v[fill, wq0:]
            want = np.zeros(n, dtype=np.int64)
            for rho, (first, slots) in enumerate(regions):
                pixels = slots - (missing if slots and g1 == first + slots else 0)
                assert 0 <= counts[rho] <= pixels
                if fill == 0:
                    assert counts[rho] == 0
                if fill == 1:
                    assert counts[rho] == pixels  # the sub-region is all retirees
                want[first:first + counts[rho]] = 1  # the front of the sub-region, nothing else
            assert np.array_equal(is_retiree, want), (f, fill)
            assert is_retiree.sum() == counts.sum()  # one slot per retiree: none twice, none missing
            if missing:
                gaps += 1
                assert not is_retiree[g0:g1].any()  # ... and a front that fills its sub-region's pixels ends where the gap begins
                if fill == 1:
                    assert g0 > 0 and is_retiree[g0 - 1]
    assert gaps > 100
