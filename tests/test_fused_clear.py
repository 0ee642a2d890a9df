"""GPU (-m gpu): sdt_gpu_reset leaves the node table's clear as a debt that the first launches of the level-1 scatter pay off
(csrc/sdt_clear_plan.h, SkFuse of csrc/sdt_sk_scatter_seq.cuh); whoever else needs the table first settles it with k_clear.

Every scenario counts job A, calls reset and then looks at the table -- mostly by counting job B, other reads, and comparing every
node, the histogram and `linear` with the oracle of B alone, before and after delow(2) (tests/fused_clear_util.py).  A slot that the
deferred clear misses shows up as a node of A.  `host_cleared_slots` of stage_times says how many slots were left for k_clear since
the reset; the expected figures follow from the plan: a tile of 256 reads stores units of 256 slots, at most 128 KB of them (25 units
of a 1-word table, 18 with first ordinals, 14 of a 2-word table).

  all_by_tiles   4 000 reads of 150 bases (16 tiles), K = 31, 2^16 slots: the tiles clear all of it
  cap            the same reads and 2^22 slots: the cap leaves most of the table to the host
  three_pushes   three pushes (6 tiles each) after one reset: the debt is carried from launch to launch
  ragged         66 672 slots (SDT_TABLE_SLOT_ROUND): 260 units for the tiles, 112 slots for the host
  first          SDT_FLAG_TRACK_FIRST, small and large table
  k63            2-word keys
  pool48         SDT_SK_POOL_CHUNKS1=48 (children of their own): runs find no chunk in a fused launch, are cut, and replayed through
                 the direct path -- with the table all cleared by the tiles, and with debt left that a k_clear settles on the device
  empty / search / import / direct / reset2
                 reset followed directly by finish_count + mark_and_hist, a k-mer search, import_nodes, a job that takes the direct
                 family, a second reset
Every scenario also runs with SDT_LAZY_CLEAR=0 (reset clears the table itself) and must return the same bytes.  Integer work: bit-exact."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import fullsize_paths_util as fu
import fused_clear_util as fc

pytestmark = pytest.mark.gpu

PART, FIRST = 2, 4                                           # SDT_FLAG_PARTITION, SDT_FLAG_TRACK_FIRST
NB, NA_SMALL = 4000, 300
SMALL, BIG, RAGGED = 1 << 14, 1887437, 30000                  # est_distinct -> 2^16, 2^22 and 66 672 slots
UNIT = 256


def scenarios():
    one = [[0, NB]]
    sc = lambda name, **kw: dict(dict(name=name, K=31, flags=PART, est_distinct=SMALL, a=[0, NA_SMALL], kind="count", pushes=one, ans="b31_"), **kw)
    return [
        sc("all_by_tiles"),
        sc("cap", est_distinct=BIG, a=[0, NB]),
        sc("three_pushes", est_distinct=BIG, a=[0, NB], pushes=[[0, 1400], [1400, 2700], [2700, NB]]),
        sc("ragged", est_distinct=RAGGED),
        sc("first", flags=PART | FIRST),
        sc("first_cap", flags=PART | FIRST, est_distinct=BIG, a=[0, NB]),
        sc("k63", K=63, ans="b63_"),
        sc("empty", kind="empty"),
        sc("search", kind="search"),
        sc("import", kind="import"),
        sc("direct", flags=0),
        sc("reset2", kind="reset2"),
    ]


def pool_scenarios():
    sc = lambda name, **kw: dict(dict(name=name, K=31, flags=PART, est_distinct=SMALL, a=[0, NA_SMALL], kind="count", pushes=[[0, NB]], ans="b31_"), **kw)
    return [sc("pool48"), sc("pool48_cap", est_distinct=BIG, a=[0, NB]), sc("pool48_first", flags=PART | FIRST)]


@functools.lru_cache(maxsize=None)
def arrays():
    from soapdenovo_trans_amd import synth
    ta = synth.make_transcriptome(40, seed=101)
    ac, ao = synth.sample_reads(*ta, n_reads=NB, read_len=150, seed=102)
    tb = synth.make_transcriptome(8, seed=202, lo=500, hi=1500)
    bc, bo = synth.sample_reads(*tb, n_reads=NB, read_len=150, seed=203, err=0.001)
    out = dict(a_codes=ac, a_offs=ao, b_codes=bc, b_offs=bo)
    for K in (31, 63):
        for k, v in fu.oracle_answer(ob, K, [(bc, bo)], with_first=True).items():
            out[f"b{K}_{k}"] = v
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def lazy(tmp_path_factory, pkg):
    return fc.run_child(tmp_path_factory.mktemp("fused_on"), "on", {"SDT_TABLE_SLOT_ROUND": 8}, scenarios(), arrays())


@pytest.fixture(scope="module")
def eager(tmp_path_factory, pkg):
    return fc.run_child(tmp_path_factory.mktemp("fused_off"), "off", {"SDT_TABLE_SLOT_ROUND": 8, "SDT_LAZY_CLEAR": 0}, scenarios(), arrays())


@pytest.fixture(scope="module")
def lazy_pool(tmp_path_factory, pkg):
    return fc.run_child(tmp_path_factory.mktemp("pool_on"), "pool_on", {"SDT_SK_POOL_CHUNKS1": 48}, pool_scenarios(), arrays())


@pytest.fixture(scope="module")
def eager_pool(tmp_path_factory, pkg):
    return fc.run_child(tmp_path_factory.mktemp("pool_off"), "pool_off", {"SDT_SK_POOL_CHUNKS1": 48, "SDT_LAZY_CLEAR": 0}, pool_scenarios(), arrays())


def tiles(n):
    return (n + 255) // 256


# slots the tiles cannot take: what the plan leaves for the host (units per tile = the share rounded up, capped)
def left_for_host(slots, pushes, cap):
    for r0, r1 in pushes:
        units = slots // UNIT if slots > 0 else 0
        t = tiles(r1 - r0)
        per_tile = min(cap, -(-units // t))
        slots -= min(units, per_tile * t) * UNIT
    return slots


EXPECT = {                                                   # name -> (slots, slots left for k_clear)
    "all_by_tiles": (1 << 16, 0),
    "cap": (1 << 22, (1 << 22) - 16 * 25 * UNIT),
    "three_pushes": (1 << 22, (1 << 22) - 18 * 25 * UNIT),
    "ragged": (66672, 112),
    "first": (1 << 16, 0),
    "first_cap": (1 << 22, (1 << 22) - 16 * 18 * UNIT),
    "k63": (1 << 16, (1 << 16) - 16 * 14 * UNIT),
    "reset2": (1 << 16, 0),
}


def test_the_expected_figures_follow_from_the_plan():
    by_name = {s["name"]: s for s in scenarios()}
    for name, (slots, left) in EXPECT.items():
        s = by_name[name]
        cap = 14 if s["K"] == 63 else 18 if s["flags"] & FIRST else 25
        assert left_for_host(slots, s["pushes"], cap) == left, name


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_the_scatter_clears_what_the_plan_says(lazy, name):
    res = lazy[name]
    slots, left = EXPECT[name]
    print(name, res)
    assert res["slots"] == slots, (name, res["slots"])
    assert res["counters"]["host_cleared_slots"] == left, (name, res["counters"]["host_cleared_slots"], left)
    assert res["counters"]["pool_direct"] == 0 and res["scatter_ms"] > 0 and res["direct_ms"] == 0, (name, res)


@pytest.mark.parametrize("name", ["empty", "search", "import", "direct"])
def test_whoever_comes_first_after_reset_sees_an_empty_table(lazy, name):
    res = lazy[name]
    print(name, res)
    assert res["counters"]["host_cleared_slots"] == res["slots"] == 1 << 16, (name, res)     # nothing fused: k_clear took the whole table
    if name == "direct":
        assert res["direct_ms"] > 0 and res["scatter_ms"] == 0 and res["counters"]["batches"] == 0, res


@pytest.mark.parametrize("name", [s["name"] for s in scenarios()])
def test_the_switch_off_returns_the_same(lazy, eager, name):
    on, off = lazy[name], eager[name]
    assert off["counters"]["host_cleared_slots"] == off["slots"] == on["slots"], (name, off)      # reset cleared the table itself
    assert on.get("digest") == off.get("digest"), name
    same = lambda c: {k: c[k] for k in ("pool_direct", "batches", "batch_kmers", "records", "lds_spills")}      # (the others depend on which workgroup took which tile)
    assert same(on["counters"]) == same(off["counters"]), (name, on["counters"], off["counters"])


@pytest.mark.parametrize("name", [s["name"] for s in pool_scenarios()])
def test_runs_without_a_chunk_are_replayed(lazy_pool, eager_pool, name):
    on, off = lazy_pool[name], eager_pool[name]
    print(name, on, off)
    for res in (on, off):
        assert 0 < res["counters"]["pool_direct"] <= res["kmers"], (name, res)
    # with the table all cleared by the tiles the host has nothing to do; where the cap leaves debt the host still launches its k_clear for
    # it (and the device skips it: the replay's conditional clear was there first)
    assert on["counters"]["host_cleared_slots"] == (0 if on["slots"] == 1 << 16 else on["slots"] - 16 * 25 * UNIT), (name, on)
    # (pool_direct itself differs: a fused launch cuts a read at its first run without a chunk, the plain one tries every run)
    assert on["digest"] == off["digest"], name
