"""The first-bounce rule of csrc/pt_sched.h without a GPU: the fits that make the host fall back to split records, and how the
words of that form are packed.  (Which batches store one record per surviving pixel and batch and leave the first bounce to k_paths
is a rung of batch_form: tests/test_sched_form.py.)

The record's last word holds the tile pixel below the material index (pack_first); the word that waits beside a record in a lane's
refill slot holds the iteration of its sub-list above the visit number modulo 2^kVisitBits (pack_visit), and k_paths compares visit
numbers modulo that width (visit_gap): a path in flight was taken at most kVisitRing visits ago, so the comparison must hold over
every wrap.  tests/sched_first_bounce_driver.cpp, built with the system compiler, prints the header's functions over a sweep; here
they are checked by enumeration."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """{case name: [fields]} of the driver's output."""
    exe = str(tmp_path_factory.mktemp("sched_first_bounce") / "sched_first_bounce_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_first_bounce_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # the header compiles as plain C++, without warnings
    text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    cases = {}
    for line in text.splitlines():
        name, *tokens = line.split()
        cases.setdefault(name, []).append({k: int(v) for k, v in (t.split("=") for t in tokens)})
    return cases


def test_fallbacks_for_words_that_do_not_fit(out):
    for f in out["fits"]:
        assert f["ok"] == int(f["mats"] <= 1 << (31 - f["shift"])), f
    assert {f["shift"] for f in out["fits"]} == set(range(1, 31)) and {f["ok"] for f in out["fits"]} == {0, 1}
    (c,), = [out["consts"]]
    for f in out["kfits"]:
        assert f["ok"] == int(f["K"] <= 1 << (31 - c["visit_bits"])), f
    assert [f["ok"] for f in out["kfits"]] == [1, 1, 1, 1, 1, 1, 0]  # 65 and 256 iterations fit: K is not held to the 64 lanes


def test_packed_words_round_trip(out):
    for f in out["first"]:
        assert f["word"] == (f["mat"] << f["shift"]) | f["pl"] and 0 <= f["word"] < 2 ** 31
        assert (f["out_pl"], f["out_mat"]) == (f["pl"], f["mat"]), f
    assert {f["shift"] for f in out["first"]} == set(range(1, 31))
    (c,), = [out["consts"]]
    width = 1 << c["visit_bits"]
    for f in out["visit"]:
        assert f["word"] == (f["k"] << c["visit_bits"]) | (f["visit"] % width) and f["word"] < 2 ** 31  # rides in an int
        assert f["out_k"] == f["k"] and f["out_visit"] == f["visit"] % width, f
    assert any(f["visit"] >= width for f in out["visit"])


def test_lap_comparison_holds_over_a_wrap(out):
    (c,), = [out["consts"]]
    width = 1 << c["visit_bits"]
    assert c["visit_ring"] < width  # every distance a path in flight can have is told apart
    wrapped = 0
    for f in out["gap"]:
        assert f["gap"] == f["ahead"], f  # the true distance, although only the visit number modulo the width was kept
        wrapped += f["now"] // width != f["then"] // width
    assert wrapped > 100 and max(f["ahead"] for f in out["gap"]) == c["visit_ring"]
