"""The gather plan of csrc/pt_sched.h without a GPU: for each batch of a render call, which gather it gets, whether its k_paths
gathers the batch before it, whether its own gather waits for the batch after it, which of the two record planes it writes, what
PtStats.gather_form reports and which launch closes it.

The rule that matters most is the plane: a batch whose gather waits takes plane `after` mod 2 and a batch that gathers its predecessor
takes the plane that one left free, so that nothing waits and the last batch lies in plane 0 when a render call returns.
tests/sched_gather_driver.cpp, built with the system compiler, steps gather_plan through every render call of 1 to 6 batches — second
plane present or not, convergence metric off, on or on in the odd batches, the primary key the same or not at every batch, every set of
the four switches that shape the gather, fused bounces or not, nothing waiting at the start or a batch waiting in either plane — feeding
each batch's plan in as the next batch's waiting state.  Here the chains are checked by enumeration against a restatement of the plan."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
BY_VISIT, TILE_GATHER, EVERY_BATCH, GATHER_EVERY_BATCH = 16384, 32768, 65536, 131072  # PtOptions.debug_flags
TILE, TILE_FIXED, STREAM, INLINE = 0, 1, 2, 3  # PtStats.gather_form


@pytest.fixture(scope="module")
def calls(tmp_path_factory):
    """{n: {column: array of shape (render calls of n batches, n)}} and the closing launches' numbers."""
    exe = str(tmp_path_factory.mktemp("sched_gather") / "sched_gather_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_gather_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # the header compiles as plain C++, without warnings
    head, closings, body = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n", 2)
    cols = head.split("=")[1].split(",")
    v = np.array(body.split(), dtype=np.int64).reshape(-1, len(cols))
    by_n = {}
    for n in range(1, 7):
        rows = v[v[:, cols.index("n")] == n].reshape(-1, n, len(cols))  # the driver prints a call's batches in order, call after call
        by_n[n] = {c: rows[:, :, j] for j, c in enumerate(cols)}
        assert (by_n[n]["chain"] == by_n[n]["chain"][:, :1]).all() and (by_n[n]["i"] == np.arange(n)).all()
    names = ("stream", "stats_stream_planes", "stats_conv", "stats_tile", "stats")
    return by_n, dict(zip(names, (int(x) for x in closings.split("=")[1].split(","))))


def test_every_toggle_is_swept(calls):
    by_n, closing = calls
    assert len(set(closing.values())) == 5
    total = 0
    for n, c in by_n.items():
        assert len(c["chain"]) == 2 * 3 * 16 * 2 * 3 * 2 ** n  # plane x metric x switches x fused x start x keys
        total += len(c["chain"])
        assert (c["after"] == n - 1 - c["i"]).all()
        assert len(np.unique(c["flags"])) == 16 and set(np.unique(c["flags"] & ~(BY_VISIT | TILE_GATHER | EVERY_BATCH | GATHER_EVERY_BATCH))) == {0}
        for key in ("second_plane", "metric", "fused", "same_key", "fixed", "once", "waiting"):
            assert set(np.unique(c[key])) == {0, 1}, (n, key)
        assert set(np.unique(c["waiting_plane"][:, 0][c["waiting"][:, 0] == 1])) == {0, 1}  # a call that begins with a batch waiting in either plane
        # the ladder's part (tests/test_sched_form.py): the switches reach the plan through the batch's form
        assert np.array_equal(c["fixed"], (c["flags"] & BY_VISIT == 0).astype(np.int64))
        assert np.array_equal(c["once"], (c["flags"] & (BY_VISIT | EVERY_BATCH) == 0).astype(np.int64))
    assert total == 576 * 126


def test_the_plan_is_its_restatement(calls):
    """Each batch's plan from its inputs, restated (Host loop)."""
    by_n, closing = calls
    seen = set()
    for c in by_n.values():
        # the gather: records in order of retirement need the tile; fixed slots stream unless the switch or the metric asks for the tile
        form = np.where(c["fixed"] == 0, TILE, np.where((c["flags"] & TILE_GATHER != 0) | (c["metric"] != 0), TILE_FIXED, STREAM))
        assert np.array_equal(c["form"], form)
        # a stream gather may run inside the next batch's k_paths: depth 0 once per camera, a second plane to write meanwhile, fused bounces, no switch against it
        may = (form == STREAM) & (c["once"] != 0) & (c["second_plane"] != 0) & (c["fused"] != 0) & (c["flags"] & GATHER_EVERY_BATCH == 0)
        gathers = may & (c["waiting"] != 0) & (c["same_key"] != 0)  # ... the batch before waits and this one launches no k_primary over what that gather reads
        defers = may & (c["after"] > 0)  # ... another batch of the call follows
        assert np.array_equal(c["gathers_waiting"] != 0, gathers) and np.array_equal(c["defers"] != 0, defers)
        plane = np.where(gathers, 1 - c["waiting_plane"], np.where(defers, c["after"] & 1, 0))
        assert np.array_equal(c["plane"], plane)
        # PtStats.gather_form: 3 only while the batch waits, else how it was gathered
        assert np.array_equal(c["reported"], np.where(defers, INLINE, form))
        want = np.where(defers, closing["stats"],
                        np.where(form == STREAM, np.where(plane == 0, closing["stream"], closing["stats_stream_planes"]),
                                 np.where(c["metric"] != 0, closing["stats_conv"], closing["stats_tile"])))
        assert np.array_equal(c["closing"], want)
        seen |= set(np.unique(want).tolist())
    assert seen == set(closing.values())  # every closing launch occurs


def test_every_batch_is_gathered_once_and_nothing_waits_when_the_call_returns(calls):
    by_n, closing = calls
    deferred = not_deferred = inline = by_a_launch_first = began_waiting = 0
    for n, c in by_n.items():
        gathers, defers, waiting = c["gathers_waiting"] != 0, c["defers"] != 0, c["waiting"] != 0
        # the chain: what a batch finds waiting is what the batch before it left (run_batch), or what the call began with
        assert np.array_equal(waiting[:, 1:], defers[:, :-1])
        assert np.array_equal(c["waiting_plane"][:, 1:][defers[:, :-1]], c["plane"][:, :-1][defers[:, :-1]])
        # gathers of batch i: by its own closing launch, inside the next batch's k_paths, or by the launch run_batch issues before a batch
        # that finds one waiting and does not take it
        own = c["closing"] != closing["stats"]
        by_next = np.zeros_like(own)
        by_next[:, :-1] = waiting[:, 1:]  # (inline when the next batch gathers_waiting, by a launch first otherwise: one of the two, always)
        assert (own.astype(int) + by_next.astype(int) == 1).all()
        assert not (gathers & ~waiting).any()  # nobody gathers a batch that does not wait
        assert not defers[:, -1].any() and own[:, -1].all()  # nothing waits after the last batch
        assert (c["reported"][:, -1] != INLINE).all() and not (c["reported"] == INLINE)[~defers].any()
        # a batch that gathers its predecessor writes the other plane; nobody else reads a plane while it is written
        assert np.array_equal(c["plane"][gathers], 1 - c["waiting_plane"][gathers])
        assert ((c["plane"] == 0) | (c["second_plane"] != 0)).all()  # plane 1 only where it exists
        # where did the chain each batch belongs to begin?  (-1: with the batch that waited when the call began)
        began = np.zeros_like(c["i"])
        for i in range(n):
            began[:, i] = np.where(gathers[:, i], began[:, i - 1] if i else -1, i)
        inside = began[:, -1] >= 0
        assert (c["plane"][:, -1][inside] == 0).all()  # a call's last batch writes plane 0 whenever its chain began inside the call
        assert (c["closing"][:, -1][inside & (c["form"][:, -1] == STREAM)] == closing["stream"]).all()  # ... and is gathered with the counter rows in one launch
        # along a chain that began inside the call the planes are `after` mod 2
        assert np.array_equal(c["plane"][gathers & (began >= 0)], (c["after"] & 1)[gathers & (began >= 0)])
        deferred += int(defers.sum())
        not_deferred += int((~defers & (c["form"] == STREAM)).sum())
        inline += int(gathers.sum())
        by_a_launch_first += int((waiting & ~gathers).sum())
        began_waiting += int((~inside).sum())
    assert min(deferred, not_deferred, inline, by_a_launch_first, began_waiting) > 0  # each case occurs: the sweep decides nothing by leaving one out
