"""CPU: the trim entry points exist at every layer (header, library, binding), and the Python restatement of the rule and of the
ranged compaction (read_trim_util.py) -- what the GPU tests expect -- does what the rule says on hand-made cases and on a population
with planted errors, on its own."""
import collections
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import read_correct_util as rc
import read_trim_util as rt
from test_kmer_search import canon_kmers
from test_read_select_host import length_mix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_trim_reads", "sdt_gpu_trim_reads_device", "sdt_gpu_trim_kept_reads", "sdt_gpu_compact_trimmed",
           "sdt_gpu_compact_trimmed_device"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_five_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    assert re.search(r"#define\s+SDT_TRIM_CORRECTED\s+1u?\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+kmers,\s*weak,\s*median,\s*start,\s*len,\s*verdict;\s*\}\s*sdt_read_trim;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+min_count,\s*min_cov,\s*min_len,\s*flags;\s*\}\s*sdt_trim_params;", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_read_trim_dtype_and_params_are_the_c_structs(pkg):
    import ctypes
    dt = pkg.READ_TRIM_DTYPE
    assert dt.itemsize == 24 == pkg.READ_COV_DTYPE.itemsize
    assert dt.names == ("kmers", "weak", "median", "start", "len", "verdict") == rt.TRIM_FIELDS and dt == rt.TRIM_DTYPE
    assert all(dt.fields[n][0] == np.uint32 and dt.fields[n][1] == 4 * i for i, n in enumerate(dt.names))
    assert ctypes.sizeof(pkg.TrimParams) == 16
    assert [(f, getattr(pkg.TrimParams, f).offset) for f, _ in pkg.TrimParams._fields_] == [("min_count", 0), ("min_cov", 4), ("min_len", 8), ("flags", 12)]
    assert (pkg.TRIM_WHOLE, pkg.TRIM_GATED, pkg.TRIM_TRIMMED, pkg.TRIM_DROPPED, pkg.TRIM_SHORT, pkg.TRIM_CORRECTED) == \
        (rt.WHOLE, rt.GATED, rt.TRIMMED, rt.DROPPED, rt.SHORT, rt.CORRECTED)
    for m in ("trim_reads", "trim_reads_device", "trim_kept_reads", "compact_trimmed", "compact_trimmed_device"):
        assert callable(getattr(pkg.PregraphGPU, m))


# ---- the rule, one hand case per line of the table ------------------------------------------------------------------------------------
K5 = 5


def by_counts(counts, min_count=2, min_cov=0, min_len=0, K=K5):
    """a read of len(counts) + K - 1 bases whose k-mers have these counts (flag off: the bases do not matter)"""
    codes = np.zeros(len(counts) + K - 1 if counts else K - 1, dtype=np.uint8)
    return rt.trim_read(codes, K, None, (min_count, min_cov, min_len, 0), kmer_counts=list(counts) if counts else None)


def test_rule_hand_cases():
    # 4 short: n == 0, whatever the settings
    assert rt.trim_read(np.zeros(K5 - 1, dtype=np.uint8), K5, None, (2, 9, 9, 0)) == (0, 0, 0, 0, 0, rt.SHORT)
    assert rt.trim_read(np.zeros(0, dtype=np.uint8), K5, None, (2, 0, 0, 0)) == (0, 0, 0, 0, 0, rt.SHORT)
    # 0 whole: nothing weak; min_count == 0 means nothing is weak, even absent k-mers; whole comes before gated and before min_len
    assert by_counts([3, 2, 7]) == (3, 0, 3, 0, 7, rt.WHOLE)
    assert by_counts([0, 0, 0], min_count=0) == (3, 0, 0, 0, 7, rt.WHOLE)
    assert by_counts([3, 2, 7], min_cov=100, min_len=100) == (3, 0, 3, 0, 7, rt.WHOLE)
    # 1 gated: the lower median below min_cov; at min_cov it is not
    assert by_counts([5, 1, 1, 5], min_cov=2) == (4, 2, 1, 0, 8, rt.GATED)
    assert by_counts([5, 1, 1, 5], min_cov=1) == (4, 2, 1, 0, 5, rt.TRIMMED)
    assert by_counts([5, 1, 5, 5], min_cov=5) == (4, 1, 5, 2, 6, rt.TRIMMED)           # (median 5 == min_cov)
    # 3 dropped: no stretch at all, or the longest covers fewer than min_len bases
    assert by_counts([1, 0, 1]) == (3, 3, 1, 0, 0, rt.DROPPED)
    assert by_counts([9, 9, 0, 9], min_len=7) == (4, 1, 9, 0, 0, rt.DROPPED)
    assert by_counts([9, 9, 0, 9], min_len=6) == (4, 1, 9, 0, 6, rt.TRIMMED)           # (2 k-mers cover K + 1 = 6 bases)
    assert by_counts([9, 0], min_len=K5) == (2, 1, 0, 0, K5, rt.TRIMMED)               # a stretch covers K bases: min_len <= K never binds
    # 2 trimmed: the longest stretch, head, interior and tail
    assert by_counts([9, 9, 9, 0, 9]) == (5, 1, 9, 0, 7, rt.TRIMMED)
    assert by_counts([0, 9, 9, 9, 0, 9, 9]) == (7, 2, 9, 1, 7, rt.TRIMMED)
    assert by_counts([9, 0, 9, 9, 9]) == (5, 1, 9, 2, 7, rt.TRIMMED)
    # ties: the first among equals, also when a longer one comes first or last
    assert by_counts([9, 9, 0, 9, 9]) == (5, 1, 9, 0, 6, rt.TRIMMED)
    assert by_counts([0, 9, 0, 9, 0, 9]) == (6, 3, 0, 1, 5, rt.TRIMMED)
    assert by_counts([9, 0, 9, 9, 0, 9, 9]) == (7, 2, 9, 2, 6, rt.TRIMMED)
    assert by_counts([9, 9, 9, 0, 9, 9, 0, 9, 9]) == (9, 2, 9, 0, 7, rt.TRIMMED)
    # weak is count < min_count, strictly
    assert by_counts([2, 1, 2], min_count=2)[1] == 1 and by_counts([2, 1, 2], min_count=3)[5] == rt.DROPPED
    # counts past 65 535 are compared as they are
    assert by_counts([70000, 70000, 66000, 66000, 66000], min_count=68000) == (5, 3, 66000, 0, 6, rt.TRIMMED)


# ---- a population with planted errors -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def population(K):
    """three transcripts counted 5 times and one counted once as a Counter, and reads of them: clean, with one to three substitutions
    anywhere (close pairs among them), junctions of two transcripts, random reads, short reads"""
    rng = np.random.default_rng(7100 + K)
    Lt = K + 120
    tx = [rng.integers(0, 4, size=Lt, dtype=np.uint8) for _ in range(4)]
    table = collections.Counter()
    for t, copies in zip(tx, (5, 5, 5, 1)):
        for k in canon_kmers(t, K):
            table[k] += copies
    reads = []
    for i in range(120):
        t = tx[i % 4]
        L = int(rng.integers(K - 2, Lt + 1))
        s = int(rng.integers(0, Lt - L + 1))
        r = t[s:s + L].copy()
        nsub = i % 4
        if nsub and L:
            first = int(rng.integers(0, L))
            gaps = (0, 1, K - 1, K, K + 1, int(rng.integers(1, L + 1)))
            for j in range(nsub):
                p = min(L - 1, first + j * gaps[(i // 4) % len(gaps)])
                r[p] = (r[p] + 1 + j) & 3
        reads.append(r if i & 8 else (r[::-1] ^ 2))
    reads.append(np.concatenate([tx[0][-(K + 9):], tx[1][:K + 30]]))
    reads.append(np.concatenate([tx[3][:K + 5], tx[2][40:K + 50]]))
    reads.append(rng.integers(0, 4, size=K + 40, dtype=np.uint8))
    return table, reads


def solid_mask(c, min_count):
    return [x >= min_count for x in c]


@pytest.mark.parametrize("K", [21, 31, 63])
def test_restatement_properties_on_planted_errors(K):
    table, reads = population(K)
    count = lambda k: table.get(k, 0)
    seen = collections.Counter()
    ties = 0
    for min_count, min_cov, min_len in ((2, 0, 0), (2, 3, 0), (2, 0, K + 25), (6, 0, 0)):
        for r in reads:
            n, weak, median, start, ln, verdict = rt.trim_read(r, K, count, (min_count, min_cov, min_len, 0))
            seen[verdict] += 1
            if len(r) < K:
                assert (n, weak, median, start, ln, verdict) == (0, 0, 0, 0, 0, rt.SHORT)
                continue
            c = [count(k) for k in canon_kmers(r, K)]
            solid = solid_mask(c, min_count)
            assert n == len(c) and weak == solid.count(False) and median == sorted(c)[(n - 1) // 2]
            runs = rc.runs_of(solid)                       # [a, b] inclusive
            longest = max((b - a + 1 for a, b in runs), default=0)
            if verdict in (rt.WHOLE, rt.GATED):
                assert (start, ln) == (0, len(r))
                assert all(solid) if verdict == rt.WHOLE else (not all(solid) and min_cov > 0 and median < min_cov)
            elif verdict == rt.DROPPED:
                assert (start, ln) == (0, 0) and not all(solid) and not (min_cov > 0 and median < min_cov)
                assert longest == 0 or longest + K - 1 < min_len
            else:
                assert verdict == rt.TRIMMED and not all(solid) and not (min_cov > 0 and median < min_cov)
                s = ln - K + 1
                assert s >= 1 and ln >= min_len and start + ln <= len(r)
                assert all(solid[start:start + s])                                      # every k-mer of the kept part is solid
                assert (start == 0 or not solid[start - 1]) and (start + s == n or not solid[start + s])        # the stretch is maximal
                assert s == longest                                                     # no other stretch is longer
                assert not any(b - a + 1 == s and a < start for a, b in runs)           # an equal earlier stretch would have won
                ties += sum(b - a + 1 == s for a, b in runs) > 1
    assert set(seen) == {rt.WHOLE, rt.GATED, rt.TRIMMED, rt.DROPPED, rt.SHORT}, seen


def test_a_tie_goes_to_the_first_stretch_on_real_reads():
    """one substitution in the very middle of a full-length read of odd length leaves two stretches of equal length"""
    K = 21
    rng = np.random.default_rng(1)
    t = rng.integers(0, 4, size=K + 120, dtype=np.uint8)
    local = collections.Counter({k: 4 for k in canon_kmers(t, K)})
    r = t.copy()
    L = len(r)
    assert L & 1
    r[(L - 1) // 2] ^= 1
    rec = rt.trim_read(r, K, lambda k: local.get(k, 0), (2, 0, 0, 0))
    half = (L - 1) // 2
    assert rec == (L - K + 1, K, 4, 0, half, rt.TRIMMED)
    assert rt.trim_read(r[::-1] ^ 2, K, lambda k: local.get(k, 0), (2, 0, 0, 0))[3:] == (0, half, rt.TRIMMED)


# ---- the flag -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [21, 31, 63])
def test_flag_equals_trimming_the_corrected_read(K):
    """at min_cov = 0: trimming the read as it came with SDT_TRIM_CORRECTED gives the start, len and verdict of trimming the corrected
    read without it -- a substitution at p changes exactly the k-mers of its own run"""
    table, reads = population(K)
    count = lambda k: table.get(k, 0)
    fixed = differ = 0
    for min_count, min_len in ((2, 0), (2, K + 25), (6, 0)):
        for r in reads:
            with_flag = rt.trim_read(r, K, count, (min_count, 0, min_len, rt.CORRECTED))
            rec, subs = rc.correct_read(r, K, count, min_count)
            corrected = r.copy()
            for p, x in subs:
                corrected[p] = x
            plain = rt.trim_read(corrected, K, count, (min_count, 0, min_len, 0))
            assert with_flag[3:] == plain[3:], (K, min_count, min_len, with_flag, plain, subs)
            # weak and median describe the read as it came
            without = rt.trim_read(r, K, count, (min_count, 0, min_len, 0))
            assert with_flag[:3] == without[:3]
            fixed += len(subs)
            differ += with_flag[3:] != without[3:]
            if not subs:
                assert with_flag == without
    assert fixed > 20 and differ > 10


# ---- the ranged compaction ----------------------------------------------------------------------------------------------------------
def range_sets(offs, seed=5):
    """records for length_mix(): whole reads, nothing, random ranges (starts in mid-word, len 0 among them), tails, single bases"""
    n = len(offs) - 1
    lens = np.diff(offs.astype(np.int64))
    rng = np.random.default_rng(seed)

    def recs(start, ln):
        t = np.zeros(n, dtype=rt.TRIM_DTYPE)
        t["start"], t["len"] = start, ln
        t["verdict"] = np.where(np.asarray(ln) > 0, rt.TRIMMED, rt.DROPPED)
        return t

    start = np.array([int(rng.integers(0, L + 1)) for L in lens])
    ln = np.array([int(rng.integers(0, L - s + 1)) for L, s in zip(lens, start)])
    ln[::5] = 0
    tails = np.minimum(lens, 3)
    return {"whole reads": recs(0, lens), "all dropped": recs(0, 0 * lens), "random ranges": recs(start, ln),
            "the last bases": recs(lens - tails, tails), "one base in the middle": recs(lens // 2, np.minimum(lens, 1)),
            "only the last read": recs(0, np.where(np.arange(n) == n - 1, lens, 0))}


def test_ranged_compaction_restatement_equals_the_per_base_reference():
    codes, offs = length_mix()
    words = rt.pack_words(codes)
    for name, trim in range_sets(offs).items():
        got_w, got_o = rt.expect_compact_trimmed(words, offs, trim)
        want_w, want_o = rt.compact_trimmed_by_bases(words, offs, trim)
        assert got_o.tolist() == want_o.tolist(), name
        assert got_w.tolist() == want_w.tolist(), name
        assert (got_w[-4:] == 0).all()
        if name == "whole reads":
            assert got_w.tolist() == words.tolist() and got_o.tolist() == sorted(set(offs.tolist()))    # (reads of 0 bases are left out)
        if name == "all dropped":
            assert got_o.tolist() == [0] and got_w.tolist() == [0, 0, 0, 0]
    r = range_sets(offs)["random ranges"]
    assert ((r["start"] + offs[:-1].astype(np.int64)) % 16 != 0).sum() > 10 and (r["len"] == 0).sum() > 5 and (r["len"] > 16).sum() > 3
    # ranges past the read are clamped to it by the restatement of the device form
    wild = r.copy()
    wild["start"][3], wild["len"][4] = 1000, 1000
    cl = rt.clamp_ranges(offs, wild)
    L3, L4 = int(offs[4] - offs[3]), int(offs[5] - offs[4])
    assert cl[3] == (L3, 0) and cl[4] == (int(wild["start"][4]), L4 - int(wild["start"][4]))


# ---- the device-free half of `sdt-kmers trim` -----------------------------------------------------------------------------------------
def test_routing_and_record_line_clean_under_sanitizers(tmp_path):
    """tools/trim_host_check.c: where a read goes given its own record, its mate's and the pair ranges, and its record line
    (csrc/host/trimsplit.c), a stand-alone program built with AddressSanitizer + UBSan and run on the CPU"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "trim_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "trim_host_check.c"), os.path.join(host, "trimsplit.c"),
                    os.path.join(host, "normsplit.c")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "trim_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_cli_texts_route_orphans_to_the_singles():
    codes = np.arange(40, dtype=np.uint8) & 3
    offs = np.array([0, 10, 20, 30, 40], dtype=np.uint64)
    trim = np.zeros(4, dtype=rt.TRIM_DTYPE)
    trim["kmers"] = 6
    trim["start"], trim["len"], trim["verdict"] = [0, 2, 0, 1], [10, 6, 0, 9], [rt.WHOLE, rt.TRIMMED, rt.DROPPED, rt.TRIMMED]
    txt, pairs, single, tally = rt.cli_texts(codes, offs, trim, [(0, 4)])
    assert txt == "6 0 0 0 10 0\n6 0 0 2 6 2\n6 0 0 0 0 3\n6 0 0 1 9 2\n"
    assert pairs == ">1\nACTGACTGAC\n>2\nACTGAC\n" and single == ">4\nGACTGACTG\n"
    assert tally == "4 reads: 1 whole, 0 gated, 2 trimmed, 1 dropped, 0 short; 40 bases in, 25 bases out\n"
    assert rt.cli_texts(codes, offs, trim, [])[1:3] == ("", ">1\nACTGACTGAC\n>2\nACTGAC\n>4\nGACTGACTG\n")


def test_sdt_kmers_usage_knows_trim_and_polices_its_options(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stderr

    for args in ((), ("trimm",), ("trim",), ("trim", "-s", "lib.cfg")):
        code, err = run(*args)
        assert code == 255
        for word in ("sdt-kmers trim -s lib.cfg -K k", "-c min_count, default 2", "--min-cov Z, default 0", "--min-len L, default 0", "--correct",
                     "prefix.readTrim", "prefix.trim.pairs.fa", "prefix.trim.single.fa", "prefix.edits", "kmers weak median start len verdict"):
            assert word in err, f"sdt-kmers {' '.join(args)}: the usage text lacks {word!r}"
    cfg = str(tmp_path / "none.cfg")                    # (never opened: the options are refused first)
    for opt, bad in (("--min-cov", "4294967296"), ("--min-cov", "2x"), ("--min-cov", "-1"), ("--min-len", "4294967296"), ("--min-len", "1e3"),
                     ("--min-len", "")):
        code, err = run("trim", "-s", cfg, "-K", "31", opt, bad, "-o", str(tmp_path / "out"))
        assert code == 255 and opt in err and "whole number" in err, f"{opt} {bad!r}: {code} {err}"
    # the options belong to trim alone, and normalize's do not belong to trim
    for sub in ("profile", "correct", "normalize", "query"):
        for opt in (("--min-cov", "3"), ("--min-len", "50"), ("--correct",)):
            code, err = run(sub, "-s", cfg, "-K", "31", *opt, "-o", str(tmp_path / "out"))
            assert code == 255 and f"{opt[0]} belongs to trim" in err, f"{sub} {opt}: {code} {err}"
    for opt in (("--target", "5"), ("--max-cv", "100"), ("--seed", "1")):
        code, err = run("trim", "-s", cfg, "-K", "31", *opt, "-o", str(tmp_path / "out"))
        assert code == 255 and f"{opt[0]} belongs to normalize" in err
    assert not os.path.exists(str(tmp_path / "out.readTrim"))
