"""The fixed-slot rule of csrc/pt_sched.h without a GPU: where k_paths stores the retirement record of the path at list position i of
sub-list (k, rho) in a first-bounce batch, and the word that waits beside the path's record in a lane's refill slot.  (Which batches
store their records that way is a rung of batch_form, tests/test_sched_form.py; how they are gathered, tests/test_sched_gather.py.)

A slot must lie among the survivors' slots of its sub-region, behind the depth-0 retirees k_primary put at the front; no two paths
of a queue may share one; and the slot without its iteration's k * seg_cap must be the same in every iteration, because the stream
gather (k_collect_stream) adds the K records it finds at ONE offset to ONE pixel.  tests/sched_fixed_slots_driver.cpp, built with the
system compiler, prints the header's functions over a sweep; here they are checked by enumeration."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """{case name: [fields]} of the driver's header lines; out["slots"][j]["rows"]: the numbers of the lines behind header j."""
    exe = str(tmp_path_factory.mktemp("sched_fixed_slots") / "sched_fixed_slots_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_fixed_slots_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # the header compiles as plain C++, without warnings
    text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    cases = {}
    for line in text.splitlines():
        if line[0].isalpha():
            name, *tokens = line.split()
            fields = {k: (v if "," in v else int(v)) for k, v in (t.split("=") for t in tokens)}
            fields["rows"] = []
            cases.setdefault(name, []).append(fields)
        else:
            cases["slots"][-1]["rows"].append(np.array(line.split(), dtype=np.int64))
    return cases


def test_every_path_has_its_own_slot_among_the_survivors(out):
    seen = {key: set() for key in ("N", "Q", "wq0", "K", "fill")}
    partial = with_gap = paths = 0
    for c in out["slots"]:
        for key in seen:
            seen[key].add(c[key])
        assert len(c["rows"]) == c["wq0"] and c["fits"] == 1
        K, seg_cap = c["K"], c["seg_cap"]
        taken = np.zeros(K * seg_cap, bool)
        for row in c["rows"]:
            rho, first, slots, retirees, survivors = (int(v) for v in row[:5])
            slot, out_k, out_slot = row[5::3], row[6::3], row[7::3]
            assert slot.size == K * survivors
            if not slot.size:
                continue
            k, i = np.divmod(np.arange(slot.size), survivors)  # the driver's order: iteration-major
            # inside [retirees, retirees + survivors) of sub-region (k, rho), in list order ...
            assert np.array_equal(slot, k * seg_cap + first + retirees + i), c
            assert retirees + survivors <= slots and first + slots <= c["my_nq"] * 64
            if c["g1"] == first + slots:  # ... which ends before the unused slots of the tile's partial last chunk
                assert first + retirees + survivors == c["g0"]
                with_gap += c["g1"] > c["g0"]
            # ... the same offset in every iteration's region
            assert np.array_equal(slot - k * seg_cap, np.tile(slot[:survivors], K))
            # the waiting word gives back the iteration and the slot
            assert np.array_equal(out_k, k) and np.array_equal(out_slot, slot)
            assert not taken[slot].any() and np.unique(slot).size == slot.size  # nobody else's
            taken[slot] = True
            paths += slot.size
        partial += c["N"] % 64 != 0
    assert seen["N"] >= {40, 63, 64, 65, 700, 5917} and seen["Q"] == {1, 4, 256} and seen["wq0"] == {1, 3, 20} and seen["K"] == {1, 3, 25, 65}
    assert seen["fill"] == {0, 1, 2} and partial > 100 and with_gap > 100 and paths > 1_000_000


def test_waiting_word_round_trips_at_the_limits(out):
    for f in out["word"]:
        assert f["bits"] == (f["seg_cap"] - 1).bit_length() and f["word"] < 2 ** 31  # the smallest width that holds every offset; rides in an int
        assert f["word"] == (f["k"] << f["bits"]) | f["off"]
        assert f["out_k"] == f["k"] and f["out_slot"] == f["k"] * f["seg_cap"] + f["off"], f
    assert {f["seg_cap"] for f in out["word"]} >= {64, 8128, 8192, 8256, 1 << 30}
    for f in out["kfits"]:
        assert f["ok"] == int(f["K"] <= 1 << (31 - f["bits"])), f
    assert {f["ok"] for f in out["kfits"]} == {0, 1}
