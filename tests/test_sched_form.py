"""The form ladder of csrc/pt_sched.h without a GPU: batch_form decides, once per batch, whether depth 0 is shared between iterations,
whether its retirees are stored once, which record form depth 1 takes, whether retirement records get fixed slots and whether depth 0
is traced once per camera — each rung a step from the one before it.

tests/sched_form_driver.cpp, built with the system compiler, prints batch_form over the cross-product of every value the per-rung
sweeps gave a condition (they were one driver per rung once; their slices and counts are kept below).  `ladder` here restates the
whole ladder from the rationale in the header, independently of its code; the two are compared case by case."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
# PtOptions.debug_flags
TRACE_EVERY_ITERATION, EVERY_ITERATION, WHOLE_RECORDS, NO_FIRST_BOUNCE, BY_VISIT, TILE_GATHER, EVERY_BATCH, GATHER_EVERY_BATCH = 128, 1024, 4096, 8192, 16384, 32768, 65536, 131072
SHARES = [-1, 0, 1, 2, 25, 64]
FLAGS = [0, 16, 128, 1024, 1024 | 16, 2048 | 512, 4096, 4096 | 16, 8192, 8192 | 4096, 8192 | 1024, 16384, 32768, 16384 | 32768, 16384 | 16, 32768 | 8192, 65536, 65536 | 16,
         65536 | 32768, 65536 | 16384]
VMAX = 1 << 23  # iterations that fit beside the visit number: 2^(31 - kVisitBits)
KS = [1, 3, 25, 1 << 18, (1 << 18) + 1, VMAX, VMAX + 1]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """{case name: [fields]} of the driver's header lines, and out["table"][0]["rows"]: {column: array} of the lines behind `table`."""
    exe = str(tmp_path_factory.mktemp("sched_form") / "sched_form_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        os.path.join(HERE, "sched_form_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # the header compiles as plain C++, without warnings
    text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    cases, numbers = {}, []
    for line in text.splitlines():
        if line[0].isalpha():
            name, *tokens = line.split()
            cases.setdefault(name, []).append({k: (v if "," in v else int(v)) for k, v in (t.split("=") for t in tokens)})
        else:
            numbers.append(line)
    (t,), = [cases["table"]]
    cols = t["cols"].split(",")
    v = np.array(" ".join(numbers).split(), dtype=np.int64).reshape(-1, len(cols))
    t["rows"] = {c: v[:, j] for j, c in enumerate(cols)}
    return cases


def ladder(share, aa, flat, depth, flags, form, mats, K, shift, seg_cap):
    """The form of a batch, restated from the rationale of each rung (arrays or scalars)."""
    off = lambda bit: (flags & bit) == 0  # noqa: E731
    # depth 0 is shared between iterations when the camera rays are the same in all of them and the lists are per (queue, iteration)
    shares = (share > 1) & (aa == 0) & (flat == 0)
    # with a second depth, what leaves depth 0 and how is then a function of the pixel: retirees once, the invariant half of a record once
    retire_once = shares & (depth >= 2) & off(EVERY_ITERATION)
    splits = shares & (depth >= 2) & off(WHOLE_RECORDS)
    # both together leave nothing per iteration at depth 0: one record per pixel, in the LDS-table search form, while the words hold
    first = splits & retire_once & off(NO_FIRST_BOUNCE) & (form == 0) & (mats <= 1 << (31 - shift)) & (K <= VMAX)
    records = np.where(first, 2, np.where(splits, 1, 0))
    # a first-bounce batch knows each path's list position: fixed record slots, while (k, slot in region) fit one word
    fixed = first & (K <= 1 << (31 - int(seg_cap - 1).bit_length())) & off(BY_VISIT)
    # and with fixed slots nothing k_primary leaves depends on the batch
    once = fixed & off(EVERY_BATCH)
    split = np.where(fixed, 3, records)
    return dict(shares=shares, retire_once=retire_once, records=records, fixed=fixed, once=once, split=split)


def _unpack(word):
    return dict(shares=word & 1 != 0, retire_once=word >> 1 & 1 != 0, records=word >> 2 & 3, fixed=word >> 4 & 1 != 0, once=word >> 5 & 1 != 0, split=word >> 6 & 3)


@pytest.fixture(scope="module")
def table(out):
    (t,), = [out["table"]]
    r = dict(t["rows"])
    r.update(_unpack(r["direct"]))
    r["shift"], r["seg_cap"] = t["shift"], t["seg_cap"]
    return r


def _slice(r, **allowed):
    """The rows whose conditions take the listed values — one of the earlier per-rung sweeps; a condition not listed is unconstrained."""
    m = np.ones(len(r["share"]), bool)
    for key, values in allowed.items():
        m &= np.isin(r[key], values)
    return m


def test_the_switches_are_named_and_what_they_were(out):
    (c,), = [out["consts"]]
    bits = dict(trace_every_iteration=TRACE_EVERY_ITERATION, every_iteration=EVERY_ITERATION, whole=WHOLE_RECORDS, no_first=NO_FIRST_BOUNCE, by_visit=BY_VISIT, tile=TILE_GATHER,
                every_batch=EVERY_BATCH, gather_every_batch=GATHER_EVERY_BATCH)
    assert {k: c[k] for k in bits} == bits
    assert len({*bits.values(), 16, 32, 64, 256, 512, 2048}) == 14  # no other PtOptions.debug_flags bit has one of their values
    assert (c["split"], c["first"]) == (1, 2) and c["template"] not in (0, 1, 2) and c["forms"] == "0,1,2,3"
    assert c["lds_tables"] == c["search_lds_tables"] == 0 and 1 << (31 - c["visit_bits"]) == VMAX
    # exactly the switches that rule the gather inside the next k_paths out for every batch of a context
    assert c["no_second_plane"] == GATHER_EVERY_BATCH | TILE_GATHER | BY_VISIT | NO_FIRST_BOUNCE | EVERY_BATCH
    (fresh,), = [out["fresh"]]
    # `BatchInfo b{}` (the drivers, the stage helpers): every rule is off unless the host sets it; the struct is what the kernels were built for
    assert (fresh["retire_once"], fresh["split_records"], fresh["fixed_slots"], fresh["size"]) == (0, 0, 0, 80)


def test_the_ladder_is_its_restatement_over_the_whole_cross_product(table):
    r = table
    assert len(r["share"]) == 6 * 2 * 2 * 4 * len(FLAGS) * 3 * 3 * len(KS)
    for key, values in dict(share=SHARES, aa=[0, 1], flat=[0, 1], depth=[1, 2, 3, 8], flags=FLAGS, form=[0, 1, 2], mats=[1, 8, 9], K=KS).items():
        assert sorted(set(r[key].tolist())) == sorted(values), key
    want = ladder(r["share"], r["aa"], r["flat"], r["depth"], r["flags"], r["form"], r["mats"], r["K"], r["shift"], r["seg_cap"])
    for key, v in want.items():
        assert np.array_equal(r[key], v), key
        assert len(np.unique(v)) > 1, key  # on and off (or every value) somewhere
    # filled from a BatchInfo the inputs, and so the form, are the same; primary_shares(BatchInfo) is the first rung
    assert np.array_equal(r["through_b"], r["direct"] & 0xff) and np.array_equal(r["direct"] >> 8 != 0, r["shares"])


def test_each_rung_stands_on_the_one_before_it(table):
    r = table
    first, splits = r["records"] == 2, r["records"] >= 1
    chain = [r["once"], r["fixed"], first, splits & r["retire_once"], r["shares"]]  # once => fixed => first => (split and retire_once) => shares
    for upper, lower in zip(chain, chain[1:]):
        assert not (upper & ~lower).any()
        assert (lower & ~upper).any()  # ... and is a step of its own: the rung below holds somewhere without it
    assert np.array_equal(r["split"], np.where(r["fixed"], 3, r["records"]))  # k_paths' SPLIT argument


def test_which_batches_retire_once(table):
    r = table
    m = _slice(r, flags=[0, 128, 1024, 1024 | 16, 2048 | 512], form=[0], mats=[1], K=[1])
    assert m.sum() == 6 * 2 * 2 * 4 * 5
    want = (r["share"] > 1) & (r["aa"] == 0) & (r["flat"] == 0) & (r["depth"] >= 2) & (r["flags"] & 1024 == 0)
    assert np.array_equal(r["retire_once"][m], want[m])
    assert want[m].sum() == 3 * 3 * 3  # share 2, 25, 64 x depth 2, 3, 8 x the three flag words without bit 1024
    # off for trace_depth 1, for jitter, for the flat lists, for primary_share <= 1 and with bit 1024, whatever else holds
    never = (r["depth"] == 1) | (r["aa"] != 0) | (r["flat"] != 0) | (r["share"] <= 1) | (r["flags"] & 1024 != 0)
    assert not r["retire_once"][never].any()


def test_which_batches_split_their_records(table):
    r = table
    m = _slice(r, flags=[0, 128, 1024, 4096, 4096 | 16, 2048 | 512], form=[1], mats=[9], K=[VMAX + 1])  # (a form, a material count and a K that rule the next rung out)
    assert m.sum() == 6 * 2 * 2 * 4 * 6
    want = (r["share"] > 1) & (r["aa"] == 0) & (r["flat"] == 0) & (r["depth"] >= 2) & (r["flags"] & WHOLE_RECORDS == 0)
    assert np.array_equal(r["records"][m], want[m].astype(np.int64))
    assert want[m].sum() == 3 * 3 * 4  # share 2, 25, 64 x depth 2, 3, 8 x the four flag words without bit 4096
    same = m & (r["flags"] & (WHOLE_RECORDS | EVERY_ITERATION) == 0)
    assert np.array_equal(r["records"][same] >= 1, r["retire_once"][same])  # the conditions of retire_once, with a switch of its own
    never = (r["depth"] == 1) | (r["aa"] != 0) | (r["flat"] != 0) | (r["share"] <= 1) | (r["flags"] & WHOLE_RECORDS != 0)
    assert not r["records"][never].any()


def test_which_batches_leave_the_first_bounce_to_k_paths(table):
    r = table
    m = _slice(r, share=[-1, 1, 2, 64], depth=[1, 2, 8], flags=[0, 16, 128, 1024, 4096, 8192, 8192 | 4096, 8192 | 1024], K=[1, 25, VMAX, VMAX + 1])
    assert m.sum() == 4 * 2 * 2 * 3 * 8 * 3 * 3 * 4
    shared = (r["share"] > 1) & (r["aa"] == 0) & (r["flat"] == 0) & (r["depth"] >= 2)
    split, once = shared & (r["flags"] & WHOLE_RECORDS == 0), shared & (r["flags"] & EVERY_ITERATION == 0)
    assert np.array_equal(r["retire_once"][m], once[m])
    want = split & once & (r["flags"] & NO_FIRST_BOUNCE == 0) & (r["form"] == 0) & (r["mats"] <= 1 << (31 - r["shift"])) & (r["K"] <= VMAX)
    assert np.array_equal(r["records"][m], np.where(want, 2, split.astype(np.int64))[m])  # the fallback is the split form wherever that one holds
    # share 2, 64 x depth 2, 8 x flags 0, 16, 128 (bit 128 acts through the share the host passes) x the LDS-table form x 1 or 8
    # materials x the three K that fit
    assert want[m].sum() == 2 * 2 * 3 * 2 * 3


def test_which_batches_use_fixed_slots_and_which_gather(table):
    r = table
    m = _slice(r, share=[1, 64], depth=[1, 8], flags=[0, 16, 8192, 4096, 1024, 16384, 32768, 16384 | 32768, 16384 | 16, 32768 | 8192], form=[0, 1], mats=[8, 9],
               K=[25, 1 << 18, (1 << 18) + 1])
    assert 2 * m.sum() == 2 * 2 * 2 * 2 * 10 * 2 * 2 * 3 * 2  # (each row with and without the convergence metric)
    shared = (r["share"] > 1) & (r["aa"] == 0) & (r["flat"] == 0) & (r["depth"] >= 2)
    first = shared & (r["flags"] & (WHOLE_RECORDS | EVERY_ITERATION | NO_FIRST_BOUNCE) == 0) & (r["form"] == 0) & (r["mats"] <= 8) & (r["K"] <= 1 << 23)
    assert np.array_equal((r["records"] == 2)[m], first[m])
    fits = r["K"] <= 1 << (31 - (r["seg_cap"] - 1).bit_length())
    want = first & fits & (r["flags"] & BY_VISIT == 0)  # false exactly when the first-bounce rung is, the bit is set or the word does not fit
    assert np.array_equal(r["fixed"][m], want[m])
    on = {0: 0, 1: 0, 2: 0}
    for conv, col in ((0, "gather"), (1, "gather_metric")):
        gather = np.where(~want, 0, np.where((r["flags"] & TILE_GATHER != 0) | (conv != 0), 1, 2))
        assert np.array_equal(r[col], gather)  # (over the whole table, not this slice alone)
        for form in on:
            on[form] += int((gather[m] == form).sum())
    assert min(on.values()) > 0
    # (K = 2^18 + 1 fits beside the visit number and not beside the slot: the word alone turns the rule off there)
    assert (m & first & ~r["fixed"] & (r["flags"] & BY_VISIT == 0)).any()


def test_which_batches_read_an_earlier_batch_s_first_hits(table):
    r = table
    m = _slice(r, share=[1, 64], depth=[1, 2, 8], flags=[0, 16, 65536, 65536 | 16, 8192, 4096, 1024, 16384, 32768, 65536 | 32768, 65536 | 16384, 128], mats=[8, 9],
               K=[1, 3, 25, 1 << 18, (1 << 18) + 1])
    assert m.sum() == 2 * 2 * 2 * 3 * 12 * 3 * 2 * 5
    shared = (r["share"] > 1) & (r["aa"] == 0) & (r["flat"] == 0) & (r["depth"] >= 2)
    first = shared & (r["flags"] & (WHOLE_RECORDS | EVERY_ITERATION | NO_FIRST_BOUNCE) == 0) & (r["form"] == 0) & (r["mats"] <= 8) & (r["K"] <= 1 << 23)
    fixed = first & (r["K"] <= 1 << 18) & (r["flags"] & BY_VISIT == 0)
    assert np.array_equal((r["records"] == 2)[m], first[m]) and np.array_equal(r["fixed"][m], fixed[m])  # the bit changes neither of the rules it stands on
    want = fixed & (r["flags"] & EVERY_BATCH == 0)
    assert np.array_equal(r["once"][m], want[m])
    assert want[m].sum() > 0 and (fixed & ~want)[m].sum() > 0 and (first & ~fixed)[m].sum() > 0  # on, off by the bit, off by the slots
    # every form whose depth 0 has per-iteration output traces in every batch: jitter, flat lists, a trace per iteration (share 1 and,
    # in the kernels, bit 128, which the host turns into share 1), depth 1, split and whole records, the other search forms
    never = (r["aa"] != 0) | (r["flat"] != 0) | (r["share"] <= 1) | (r["depth"] < 2) | (r["form"] != 0) | (r["flags"] & (NO_FIRST_BOUNCE | WHOLE_RECORDS | EVERY_ITERATION | BY_VISIT) != 0)
    assert not r["once"][never].any()


def test_a_shorter_batch_of_the_plan_qualifies_too(out):
    """The counts are published for the plan's K; a tail batch or a warm-up of fewer iterations must not fall out of the rule."""
    assert len(out["shorter"]) == 3 * 6 * 3
    for f in out["shorter"]:
        assert f["kb"] <= f["K"]
        if f["once_K"]:
            assert f["once_kb"], f
    assert {f["once_K"] for f in out["shorter"]} == {0, 1}
