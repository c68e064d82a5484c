"""The split-record rule of csrc/pt_sched.h without a GPU: where the iteration-invariant half of a depth-1 record lives, and how
the specular / diffuse bit shares a word with the sample id.  (Which batches split their records is a rung of batch_form:
tests/test_sched_form.py.)

In such a batch k_primary writes (origin, material) of a surviving pixel once, at the slot its record has in iteration 0 of the
batch, and k_paths reads it from there for the record of every iteration: invariant_slot must send slot i of sub-list (q, k, r)
to slot i of sub-list (q, 0, r), for every k, and never two records of an iteration to one slot.  The bit rides in bit 31 of the
word that holds the sample id k << slot_shift | pl, which pt_init keeps below 2^31.
tests/sched_split_records_driver.cpp, built with the system compiler, prints the header's functions over the sweep of
tests/sched_retire_once_driver.cpp; here they are checked by enumeration."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")


def _fields(tokens):
    return {k: int(v) for k, v in (t.split("=") for t in tokens)}


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """{case name: [(header fields, [number lines])]} of the driver's output."""
    exe = str(tmp_path_factory.mktemp("sched_split_records") / "sched_split_records_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_split_records_driver.cpp"), "-o", exe], capture_output=True, text=True)
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


def _sub_lists(my_nq, wq0):
    """[(first slot, slots)] of the sub-lists r = 0 .. wq0 - 1 of a region (pt_sched.h sub_offset / sub_chunks)."""
    quo, rem = divmod(my_nq, wq0)
    return [((r * quo + min(r, rem)) * 64, (quo + (1 if r < rem else 0)) * 64) for r in range(wq0)]


def test_invariant_slot_is_the_slot_of_iteration_0(out):
    by_queue = {}
    seen = set()
    for f, (line,) in out["index"]:
        v = np.array(line.split(), dtype=np.int64).reshape(-1, 2)
        at, inv = v[:, 0], v[:, 1]
        k, seg_cap, my_nq, wq0 = f["k"], f["seg_cap"], f["my_nq"], f["wq0"]
        seen.add((f["N"] % 64 != 0, wq0 > my_nq > 0, k > 0))
        assert len(v) == my_nq * 64 and f["cap"] == f["K"] * seg_cap and my_nq * 64 <= seg_cap
        # the records of iteration k lie in the queue's list (q, k), and their invariant halves in list (q, 0), each inside its own sub-list
        assert ((at >= k * seg_cap) & (at < (k + 1) * seg_cap)).all()
        pos = 0
        for first, n in _sub_lists(my_nq, wq0):
            assert ((inv[pos:pos + n] >= first) & (inv[pos:pos + n] < first + n)).all(), f
            assert np.array_equal(inv[pos:pos + n], first + np.arange(n))  # slot i of sub-list r, for the i-th record of it
            pos += n
        assert pos == len(v) and len(np.unique(inv)) == len(inv)  # distinct (r, i): distinct slots
        by_queue.setdefault((f["N"], f["Q"], wq0, f["K"], f["q"]), {})[k] = inv
    # (k, r, i) and (0, r, i) share a slot
    several = 0
    for key, per_k in by_queue.items():
        assert 0 in per_k
        for k, inv in per_k.items():
            assert np.array_equal(inv, per_k[0]), (key, k)
        several += len(per_k) > 1
    assert several > 100
    assert seen >= {(False, False, False), (False, True, True), (True, False, True), (True, True, True)}


def test_kind_bit_and_sample_id_share_a_word(out):
    shifts = set()
    for f, _ in out["kind"]:
        shifts.add(f["shift"])
        assert f["id"] == (f["k"] << f["shift"]) | f["pl"] and 0 <= f["id"] < 2 ** 31  # bit 31 is never part of an id
        assert f["word"] == f["id"] | (f["spec"] << 31)
        assert f["out_id"] == f["id"] and f["out_spec"] == f["spec"]
        assert f["out_id"] >> f["shift"] == f["k"] and f["out_id"] & ((1 << f["shift"]) - 1) == f["pl"]
    assert shifts == set(range(1, 31))
    largest = {f["shift"]: f["k"] for f, _ in out["kind"]}  # (the last line of a shift holds its largest k)
    assert all(k == min(256, 1 << (31 - s)) - 1 for s, k in largest.items())  # what pt_init allows: K <= 256 and K <= 2^(31 - slot_shift)
