"""The rule of csrc/pt_sched.h for tracing depth 0 once per camera, without a GPU: primary_once beside first_bounces and fixed_slots.

A batch may read the first-hit records an earlier batch left only if k_primary's output in it depends on neither the iteration nor
the batch's length: the first-bounce form (shared depth 0, no jitter, not flat, depth >= 2, none of the bits that ask for records per
iteration, the LDS-table search form, material and K fitting their words) with fixed record slots, and PtOptions.debug_flags 65536
not set.  tests/sched_primary_once_driver.cpp, built with the system compiler, prints the header's functions over a sweep; here they
are checked by enumeration."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
EVERY_BATCH, BY_VISIT, NO_FIRST_BOUNCE, WHOLE_RECORDS, EVERY_ITERATION, TILE_GATHER = 65536, 16384, 8192, 4096, 1024, 32768  # PtOptions.debug_flags


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """{case name: [fields]} of the driver's lines."""
    exe = str(tmp_path_factory.mktemp("sched_primary_once") / "sched_primary_once_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_primary_once_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # the header compiles as plain C++, without warnings
    text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    cases = {}
    for line in text.splitlines():
        name, *tokens = line.split()
        cases.setdefault(name, []).append({k: int(v) for k, v in (t.split("=") for t in tokens)})
    return cases


def test_the_bit_is_free_and_the_others_are_what_they_were(out):
    (c,), = [out["consts"]]
    assert c == dict(every_batch=EVERY_BATCH, by_visit=BY_VISIT, no_first=NO_FIRST_BOUNCE, whole=WHOLE_RECORDS, every_iteration=EVERY_ITERATION, tile=TILE_GATHER)
    assert len({*c.values(), 16, 32, 64, 128, 256, 512, 2048}) == 13  # no other PtOptions.debug_flags bit has its value


def test_which_batches_read_an_earlier_batch_s_first_hits(out):
    assert len(out["rule"]) == 2 * 2 * 2 * 3 * 12 * 3 * 2 * 5
    on = off_by_bit = off_by_slots = 0
    for f in out["rule"]:
        shared = f["share"] > 1 and not f["aa"] and not f["flat"] and f["depth"] >= 2
        first = int(shared and not f["flags"] & (WHOLE_RECORDS | EVERY_ITERATION | NO_FIRST_BOUNCE) and f["form"] == 0 and f["mats"] <= 8 and f["K"] <= 1 << 23)
        fixed = int(first and f["K"] <= 1 << 18 and not f["flags"] & BY_VISIT)
        assert (f["first"], f["fixed"]) == (first, fixed), f  # the bit changes neither of the rules it stands on
        want = int(fixed and not f["flags"] & EVERY_BATCH)
        assert f["once"] == f["once_b"] == want, f
        on += want
        off_by_bit += fixed and not want
        off_by_slots += first and not fixed
    assert on > 0 and off_by_bit > 0 and off_by_slots > 0
    # every form whose depth 0 has per-iteration output traces in every batch: jitter, flat lists, a trace per iteration (share 1 and,
    # in the kernels, bit 128, which the host turns into share 1), depth 1, split and whole records, the other search forms
    for f in out["rule"]:
        if f["aa"] or f["flat"] or f["share"] <= 1 or f["depth"] < 2 or f["form"] != 0 or f["flags"] & (NO_FIRST_BOUNCE | WHOLE_RECORDS | EVERY_ITERATION | BY_VISIT):
            assert not f["once"], f


def test_a_shorter_batch_of_the_plan_qualifies_too(out):
    """The counts are published for the plan's K; a tail batch or a warm-up of fewer iterations must not fall out of the rule."""
    assert len(out["shorter"]) == 3 * 6 * 3
    for f in out["shorter"]:
        assert f["kb"] <= f["K"]
        if f["once_K"]:
            assert f["once_kb"], f
    assert {f["once_K"] for f in out["shorter"]} == {0, 1}
