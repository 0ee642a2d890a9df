"""GPU (-m gpu): the state rule of the kept forms, entry point by entry point -- a characterisation, so that a change of the rule shows.

One context keeps two batches (the read-1 file of 6 first mates and 5 single reads at ordinals base, base + 2, ...; the read-2 file
of the 6 second mates at base + 1, base + 3, ...).  Every kept form is called in three states: (a) the batches pushed and not
finished, (b) a batch counted from device memory and not finished, (c) after sdt_gpu_finish_count.  What each answers is compared
with a table; a refusal names the entry point and finish_count and leaves the caller's records as they were."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 21
BASE, PAIRS, SINGLES = 3, 6, 5
TOTAL = BASE + 2 * (PAIRS + SINGLES)
RANGES = [(BASE, BASE + 2 * PAIRS)]
OK, ESTATE = "SDT_OK", "SDT_ESTATE"

# Recorded on the parent of the commit that gave the kept forms one state rule (kept_drained, csrc/sdt_readstage.hpp): what every
# entry point answered there, state by state.  The forms on the counted table and complexity_ refuse while a batch is counted and not
# synchronised; the others refuse only a batch whose launch is still queued, and a small batch is launched by its own push.
# (include/sdt_gpu.h said of all of them that they "follow the rules of sdt_gpu_kept_batches": the OK entries of (a) and (b) disagree.)
EXPECT = {
    "sdt_gpu_profile_kept_reads": {"a": ESTATE, "b": ESTATE, "c": OK},
    "sdt_gpu_correct_kept_reads": {"a": ESTATE, "b": ESTATE, "c": OK},
    "sdt_gpu_trim_kept_reads": {"a": ESTATE, "b": ESTATE, "c": OK},
    "sdt_gpu_select_kept_reads": {"a": ESTATE, "b": ESTATE, "c": OK},
    "sdt_gpu_dedup_kept_reads": {"a": OK, "b": OK, "c": OK},
    "sdt_gpu_clip_kept_reads": {"a": OK, "b": OK, "c": OK},
    "sdt_gpu_overlap_kept_pairs": {"a": OK, "b": OK, "c": OK},
    "sdt_gpu_complexity_kept_reads": {"a": ESTATE, "b": ESTATE, "c": OK},
    "sdt_gpu_screen_kept_reads": {"a": OK, "b": OK, "c": OK},
    "sdt_gpu_merge_kept_pairs": {"a": OK, "b": OK, "c": OK},
    "sdt_gpu_fetch_kept_batch": {"a": OK, "b": OK, "c": OK},
}


def _reads(rng, n):
    return [rng.integers(0, 4, size=int(rng.integers(40, 61)), dtype=np.uint8) for _ in range(n)]


def _concat(reads):
    return np.concatenate(reads), np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)


def _entries(pkg, g):
    """entry point -> (the dtype of its records, call(out)); every call goes through the Python wrapper but fetch_kept_batch, whose
    wrapper owns its output"""
    ov = np.zeros(TOTAL, dtype=pkg.READ_OVERLAP_DTYPE)        # (no overlap anywhere: nothing merges, the pad words are all the output)

    def fetch(info):
        rc = g.lib.sdt_gpu_fetch_kept_batch(g._ctx, 0, info.ctypes.data, None, 0, None, 0)
        if rc != pkg.SDT_OK:
            raise pkg.SdtError(rc, g.lib.sdt_gpu_last_error().decode())

    return {
        "sdt_gpu_profile_kept_reads": (pkg.READ_COV_DTYPE, lambda out: g.profile_kept_reads(TOTAL, out=out)),
        "sdt_gpu_correct_kept_reads": (pkg.READ_FIX_DTYPE, lambda out: g.correct_kept_reads(TOTAL, out=out)),
        "sdt_gpu_trim_kept_reads": (pkg.READ_TRIM_DTYPE, lambda out: g.trim_kept_reads(TOTAL, out=out)),
        "sdt_gpu_select_kept_reads": (pkg.READ_PICK_DTYPE, lambda out: g.select_kept_reads(TOTAL, RANGES, out=out)),
        "sdt_gpu_dedup_kept_reads": (pkg.READ_DUP_DTYPE, lambda out: g.dedup_kept_reads(TOTAL, RANGES, out=out)),
        "sdt_gpu_clip_kept_reads": (pkg.READ_CLIP_DTYPE, lambda out: g.clip_kept_reads(TOTAL, params=dict(min_overlap=8, max_err_pct=10), out=out)),
        "sdt_gpu_overlap_kept_pairs": (pkg.READ_OVERLAP_DTYPE, lambda out: g.overlap_kept_pairs(TOTAL, RANGES, out=out)),
        "sdt_gpu_complexity_kept_reads": (pkg.READ_COMPLEXITY_DTYPE, lambda out: g.complexity_kept_reads(TOTAL, out=out)),
        "sdt_gpu_screen_kept_reads": (pkg.READ_SCREEN_DTYPE, lambda out: g.screen_kept_reads(TOTAL, RANGES, out=out)),
        "sdt_gpu_merge_kept_pairs": (pkg.READ_MERGE_DTYPE, lambda out: g.merge_kept_pairs(TOTAL, ov, RANGES, out=out, out_words_cap=4)),
        "sdt_gpu_fetch_kept_batch": (np.dtype((np.uint64, 4)), fetch),
    }


def observe(pkg, synth):
    """entry point -> state -> what it answered; what holds of every refusal is asserted on the way"""
    import torch
    rng = np.random.default_rng(2110)
    r1, r2 = _reads(rng, PAIRS + SINGLES), _reads(rng, PAIRS)
    scodes, soffs = _concat([rng.integers(0, 4, size=100, dtype=np.uint8) for _ in range(2)])
    seen = {}
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        entries = _entries(pkg, g)
        assert set(entries) == set(EXPECT)

        def ask(state):
            for name, (dtype, call) in entries.items():
                out = np.full(TOTAL * dtype.itemsize // 4, 0xABABABAB, dtype=np.uint32)
                try:
                    call(out.view(dtype) if dtype.shape == () else out.view(np.uint64))
                    code = OK
                except pkg.SdtError as e:
                    code = {pkg.SDT_ESTATE: ESTATE}.get(e.code, f"code {e.code}")
                    assert code != ESTATE or (name in str(e) and "finish_count" in str(e)), f"{name} ({state}): {e}"
                    assert (out == 0xABABABAB).all(), f"{name} ({state}): refused, and wrote its records"
                print(f"{name} ({state}): {code}")
                seen.setdefault(name, {})[state] = code

        assert g.screen_load(synth.pack_2bit(scodes), soffs, [0, 1], 2, K) > 0
        for batch, b in ((r1, BASE), (r2, BASE + 1)):
            g.set_read_ordinal(b, 2)
            codes, offs = _concat(batch)
            g.push_reads(synth.pack_2bit(codes), offs)
        ask("a")
        g.finish_count()
        codes, offs = _concat(r1)
        words = synth.pack_2bit(codes)
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_o = torch.from_numpy(offs.view(np.int64)).cuda()
        g.count_reads_device(d_w, len(words), d_o, len(r1), 60)
        ask("b")
        g.finish_count()
        ask("c")
    return seen


def test_kept_forms_state_rule(pkg, synth):
    seen = observe(pkg, synth)
    assert all(v["c"] == OK for v in seen.values()), seen
    assert seen == EXPECT
