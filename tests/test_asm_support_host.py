"""CPU: the assembly evaluation exists at every layer (header, library, binding); the Python restatement of the rule (asm_support_util.py)
-- what the GPU tests expect -- against a second restatement over strings and on an example worked by hand; the named case holds what
it promises, property by property, so that no GPU test can pass vacuously; the device-free half of `sdt-kmers evaluate`
(csrc/host/asmsplit.c, and the segment starts that csrc/host/screensplit.c now records) as a stand-alone program under
AddressSanitizer + UBSan; the refusals of the command line that need no device."""
import collections
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

import asm_support_util as au

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_asm_begin", "sdt_gpu_asm_add", "sdt_gpu_asm_add_device", "sdt_gpu_asm_spectrum", "sdt_gpu_asm_end"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_five_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    for words in ("c[j] < max(min_count, 1)", "A GAP is a maximal run of weak k-mers", "the first among equals; kmers if there is none",
                  "L < K: kmers = 0, longest_at = 0", "saturating at 255", "a palindrome of even K counts once per occurrence",
                  "min(count, rows - 1) = r", "none is special-cased", "sequences, k-mers, found, solid", "A second begin starts over",
                  "out NULL: tally only", "NO limit on the length of a sequence", "the table changed since sdt_gpu_asm_begin",
                  "rows < 2 or > SDT_ASM_MAX_ROWS", "one byte per table slot", "distinct counting of assembly-only k-mers", "a k other than the table's K",
                  "sharded contexts", "a kept-read form", "any change to profile_reads or its limit", "the deleted flag ignored"):
        assert words in src, f"include/sdt_gpu.h does not say {words!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint64_t\s+sum;\s*uint32_t\s+kmers,\s*found,\s*solid,\s*gaps,\s*longest_gap,\s*longest_at;\s*\}\s*sdt_seq_support;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+min_count,\s*rows,\s*flags,\s*reserved;\s*\}\s*sdt_asm_params;", src)
    assert re.search(r"#define\s+SDT_ASM_CN_COLS\s+8\b", src) and re.search(r"#define\s+SDT_ASM_MAX_ROWS\s+1024\b", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_seq_support_dtype_and_params_are_the_c_structs(pkg):
    dt = pkg.SEQ_SUPPORT_DTYPE
    assert dt.itemsize == 32 and dt.names == au.FIELDS and dt == au.DTYPE
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 12, 16, 20, 24, 28] and dt.fields["sum"][0] == np.uint64
    assert ctypes.sizeof(pkg.AsmParams) == 16
    fields = ("min_count", "rows", "flags", "reserved")
    assert [(f, getattr(pkg.AsmParams, f).offset) for f, _ in pkg.AsmParams._fields_] == [(f, 4 * i) for i, f in enumerate(fields)]
    d = pkg.AsmParams()
    assert (d.min_count, d.rows, d.flags, d.reserved) == (2, 256, 0, 0)          # the defaults of the command line
    assert pkg.ASM_CN_COLS == au.CN_COLS == 8 and pkg.ASM_MAX_ROWS == au.MAX_ROWS == 1024
    for m in ("asm_begin", "asm_add", "asm_add_device", "asm_spectrum", "asm_end"):
        assert callable(getattr(pkg.PregraphGPU, m))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
RANK = {"A": 0, "C": 1, "T": 2, "G": 3}


def canon_text(s):
    return min(s, "".join(COMP[c] for c in reversed(s)), key=lambda t: [RANK[c] for c in t])


def by_strings(read_texts, seq_texts, K, min_count, rows):
    """the rule once more, over strings: counts, records, tally and matrix"""
    counts = collections.Counter(canon_text(r[i:i + K]) for r in read_texts for i in range(len(r) - K + 1))
    mc = max(min_count, 1)
    recs, cn = [], collections.Counter()
    for s in seq_texts:
        ks = [canon_text(s[i:i + K]) for i in range(len(s) - K + 1)]
        weak = "".join("w" if counts[k] < mc else "." for k in ks)
        runs = [(m.start(), len(m.group())) for m in re.finditer("w+", weak)]
        longest = max(runs, key=lambda r: (r[1], -r[0])) if runs else (len(ks), 0)
        recs.append((sum(counts[k] for k in ks), len(ks), sum(k in counts for k in ks), weak.count("."), len(runs), longest[1], longest[0]))
        cn.update(k for k in ks if k in counts)
    m = np.zeros((rows, au.CN_COLS), dtype=np.uint64)
    for k, c in counts.items():
        m[min(c, rows - 1), min(cn[k], 255, au.CN_COLS - 1)] += 1
    return recs, m


def int_counts(reads, K):
    return dict(collections.Counter(k for r in reads for k in au.canon_kmers(r, K)))


def test_restatement_equals_the_second_restatement():
    rng = np.random.default_rng(5)
    for K, min_count, rows in ((13, 2, 8), (14, 0, 4), (21, 3, 2), (31, 1, 16)):
        genome = rng.integers(0, 4, size=900, dtype=np.uint8)
        reads = [genome[a:a + 60] if i % 2 else au.revcomp(genome[a:a + 60]) for i, a in enumerate(rng.integers(0, 840, size=150))]
        seqs = [genome[:400], au.revcomp(genome[100:500]), au.substituted(genome[300:700], 200), rng.integers(0, 4, size=90, dtype=np.uint8),
                genome[50:50 + K - 1], genome[50:50 + K], np.zeros(0, dtype=np.uint8), np.concatenate([genome[:100], genome[600:700]])]
        want_recs, want_m = by_strings([au.text_of(r) for r in reads], [au.text_of(s) for s in seqs], K, min_count, rows)
        counts = int_counts(reads, K)
        rec, cn = au.support(seqs, K, counts, min_count)
        assert [tuple(int(x) for x in r) for r in rec.tolist()] == want_recs, K
        assert (au.spectrum(counts, cn, rows) == want_m).all(), K
        assert rec["gaps"].sum() > 3 and (rec["longest_gap"] > 0).sum() >= 3 and max(cn.values()) >= 3
        assert (au.totals(rec) == [len(seqs), sum(r[1] for r in want_recs), sum(r[2] for r in want_recs), sum(r[3] for r in want_recs)]).all()


def test_restatement_on_an_example_by_hand():
    K = 4
    a = au.codes_of
    # reads: ACGTAC twice (k-mers ACGT, CGTA, GTAC: ACGT and GTAC are palindromes of even K, CGTA is stored as ... its smaller strand)
    reads = [a("ACGTAC"), a("ACGTAC"), a("TTTTT")]
    counts = int_counts(reads, K)
    k = lambda s: au.canon_kmers(a(s), K)[0]
    assert au.canon_kmers(a("ACGT"), K) == au.canon_kmers(au.revcomp(a("ACGT")), K)          # its own reverse complement
    assert counts == {k("ACGT"): 2, k("CGTA"): 2, k("GTAC"): 2, k("AAAA"): 2} and k("TTTT") == k("AAAA") == 0 and k("CGTA") == k("TACG")
    # X holds CGTA, Y its reverse complement TACG: both strands feed one node (cn 2); ACGT in X counts once per occurrence
    X, Y, Z = a("ACGTA"), a("TACG"), a("ACGTTCGTAAAAA")
    rec, cn = au.support([X, Y], K, counts, 2)
    assert rec.tolist() == [(4, 2, 2, 2, 0, 0, 2), (2, 1, 1, 1, 0, 0, 1)]
    assert cn == {k("ACGT"): 1, k("CGTA"): 2}
    # Z: ACGT . CGTT GTTC TTCG TCGT : CGTA . GTAA TAAA : AAAA AAAA  -- two gaps, of 4 and of 2: the longest starts at k-mer 1
    rec, cn = au.support([Z], K, counts, 2, cn)
    assert rec.tolist() == [(2 + 2 + 2 + 2, 10, 4, 4, 2, 4, 1)]
    assert cn == {k("ACGT"): 2, k("CGTA"): 3, k("AAAA"): 2}
    # min_count 0 is min_count 1: an absent k-mer is weak, whatever min_count says; above every count all are weak: one gap
    assert au.support([Z], K, counts, 0)[0].tolist() == au.support([Z], K, counts, 1)[0].tolist() == [(8, 10, 4, 4, 2, 4, 1)]
    assert au.support([Z], K, counts, 3)[0].tolist() == [(8, 10, 4, 0, 1, 10, 0)]
    # equal gaps: the first stays
    assert au.seq_record([1, 9, 9, 1, 9, 9, 1], {1: 5}, 2) == (15, 7, 3, 3, 2, 2, 1)
    # L < K
    assert au.support([a("ACG"), a("")], K, counts, 2)[0].tolist() == [(0, 0, 0, 0, 0, 0, 0)] * 2
    # the matrix: rows = 3 caps the counts at 2; GTAC is held by no sequence
    m = au.spectrum(counts, cn, 3)
    assert m.sum() == 4 and m[2].tolist() == [1, 0, 2, 1, 0, 0, 0, 0]
    # saturation of the tally and the last column
    cn = au.support([np.zeros(K + 299, dtype=np.uint8)], K, counts, 2)[1]
    assert cn == {0: 255} and au.spectrum(counts, cn, 2)[1].tolist() == [3, 0, 0, 0, 0, 0, 0, 1]
    # the texts of the command line
    segs, ref_of_seq, seg_start, names, bases = au.parse_fasta([">c1 x\nACGTA\nNNtacg\n>c2\nNN\n", ">c3\nACGTTCGT\nAAAAA\n"])
    assert [au.text_of(s) for s in segs] == ["ACGTA", "TACG", "ACGTTCGTAAAAA"] and ref_of_seq == [0, 0, 2] and seg_start == [0, 7, 0]
    assert names == ["c1", "c2", "c3"] and bases == [9, 0, 13]
    rec, cn = au.support(segs, K, counts, 2)
    assert au.support_text(rec, ref_of_seq, seg_start, names, bases) == "1 c1 9 3 3 3 6 0 0 3\n2 c2 0 0 0 0 0 0 0 0\n3 c3 13 10 4 4 8 2 4 1\n"
    m = au.spectrum(counts, cn, 3)
    assert au.spectrum_text(m) == "2 1 0 2 1 0 0 0 0\n"
    assert au.summary_fields(au.totals(rec), m, 2, K) == (3, 13, 7, 7, 4, 4, 3, "7500", str(round(100 * -10 * np.log10(1 - (7 / 13) ** 0.25))))


def test_the_named_case_holds_what_it_says(synth):
    c = au.named_case(synth)
    K, seqs, at, want, counts, cn, m = c["K"], c["seqs"], c["at"], c["want"], c["counts"], c["cn"], c["matrix"]
    assert K == 31 and m.shape == (64, 8)
    # the oracle's counts are the counts of the reads
    assert counts == int_counts([c["reads"][0][int(a):int(b)] for a, b in zip(c["reads"][1][:-1], c["reads"][1][1:])], K)
    offs = au.concat(seqs)[1]
    assert {int(o) % 16 for o in offs[:-1]} == set(range(16))                   # every phase of a word
    rec = lambda name: want[at[name]]
    gaps = lambda name: au.gaps_of(au.canon_kmers(seqs[at[name]], K), counts, au.NAMED_MIN_COUNT)
    # whole transcripts are found; the revcomp'd one feeds the same nodes
    assert all(rec(f"whole{i}")["kmers"] > 400 and 10 * rec(f"whole{i}")["found"] >= 9 * rec(f"whole{i}")["kmers"] for i in range(8))
    assert tuple(rec("revcomp1"))[:5] == tuple(rec("whole1"))[:5]
    # every column, a tally of exactly 255, the cap row, a count past 65 535
    assert (m.sum(axis=0) > 0).all(), m.sum(axis=0)
    assert max(cn.values()) == 255 and cn[0] == 255 and sorted(cn.values())[-2] < 255
    assert counts[0] > 65535 and m[63].sum() >= 3 and m[63, 7] >= 1 and m[:63].sum() > 0
    assert m.sum() == len(counts) == c["nodes"]
    # the gap geometry
    assert gaps("straddle") == [(49, 31)] and gaps("ends_at_63") == [(33, 31)] and gaps("starts_at_64") == [(64, 31)]
    assert tuple(rec("straddle"))[4:] == (1, 31, 49) and tuple(rec("ends_at_63"))[4:] == (1, 31, 33) and tuple(rec("starts_at_64"))[4:] == (1, 31, 64)
    (g_at, g_len), = gaps("chimera")                                           # the k-mers across the junction, but for a chance match at its rim
    assert g_at + g_len == 200 and K - 3 <= g_len <= K - 1
    assert gaps("random") == [(0, 200)] and tuple(rec("random")) == (0, 200, 0, 0, 1, 200, 0)
    for L in (K - 1, K, K + 1, K + 62, K + 63, K + 64):
        r = rec(f"len{L}")
        assert r["kmers"] == max(L - K + 1, 0) == r["solid"] and r["longest_at"] == r["kmers"]
    assert tuple(rec(f"len{K - 1}")) == (0,) * 7
    assert rec("polyA")["kmers"] == 300 and rec("polyA")["sum"] == 300 * counts[0] > 2 ** 24
    assert rec("long")["kmers"] == 20000 - K + 1 > 16384 and rec("long")["gaps"] >= 11 and rec("long")["solid"] > 10000
    # copies: columns 3 .. 7 come from the copies, not by accident
    assert (want["sum"] > 2 ** 32).any() or want["sum"].max() > 10 ** 7
    for K2 in (23, 47, 63, 95, 127):
        r = au.reduced_case(synth, K2)
        w, cn2 = au.support(r["seqs"], K2, r["counts"], 2)
        assert max(r["counts"].values()) > 65535 and max(cn2.values()) == 255 and (w["gaps"] > 0).sum() >= 4 and (w["kmers"] == 0).sum() == 3
        assert {1, 2, 63, 64, 65} <= set(w["kmers"].tolist())


# ---- the device-free half of `sdt-kmers evaluate` ------------------------------------------------------------------------------------
def test_fold_lines_and_summary_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "asm_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "asm_host_check.c"), os.path.join(host, "asmsplit.c"),
                                               os.path.join(host, "screensplit.c"), "-lm"], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "asm_host_check: ok" in r.stdout, r.stdout + r.stderr
    # the texts it wrote for the example by hand are the restatement's
    assert (tmp_path / "hand.asmSupport").read_text() == "1 c1 9 3 3 3 6 0 0 3\n2 c2 0 0 0 0 0 0 0 0\n3 c3 13 10 4 4 8 2 4 1\n"
    assert (tmp_path / "hand.asmSpectrum").read_text() == "2 1 0 2 1 0 0 0 0\n"
    q = au.summary_fields([3, 13, 7, 7], np.array([[0] * 8, [0] * 8, [1, 0, 2, 1, 0, 0, 0, 0]], dtype=np.uint64), 2, 4)[8]
    assert (tmp_path / "hand.summary").read_text() == f"evaluate: sequences 3 kmers 13 found 7 solid 7 nodes 4 solid_nodes 4 covered 3 completeness_x100 7500 qv_x100 {q}\n"


def test_sdt_kmers_usage_knows_evaluate(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    for args in ((), ("evaluate",), ("evaluate", "-s", "lib.cfg")):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 255
        for word in ("sdt-kmers evaluate -s lib.cfg -K k", "[-c min_count, default 2] --assembly contigs.fa", "[--assembly more.fa ...]",
                     "[--rows R, default 256]", "prefix.asmSupport", "prefix.asmSpectrum", "index name bases kmers found solid sum gaps longest_gap longest_at",
                     "evaluate: sequences S kmers N found F solid V nodes D solid_nodes E covered C completeness_x100 P", "a scaffold's N runs give no"):
            assert word in r.stderr, f"sdt-kmers {' '.join(args)}: the usage text lacks {word!r}"
    cfg = str(tmp_path / "none.cfg")                    # (never opened: the options are refused first)
    out = str(tmp_path / "out")
    for sub in ("profile", "correct", "trim", "screen", "qc", "query"):
        for opt in (("--assembly", "x.fa"), ("--rows", "64")):
            r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
            assert r.returncode == 255 and f"{opt[0]} belongs to evaluate" in r.stderr, f"{sub} {opt}: {r.returncode} {r.stderr[:200]}"
    r = subprocess.run([exe, "evaluate", "-s", cfg, "-K", "31", "--assembly", "x.fa", "-r", "x.fa", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and "-r belongs to screen" in r.stderr
    # no assembly at all
    r = subprocess.run([exe, "evaluate", "-s", cfg, "-K", "31", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and "--assembly contigs.fa" in r.stderr
    # rows out of range, and rows that do not exceed min_count
    for opts, say in ((("--rows", "1"), "--rows"), (("--rows", "1025"), "--rows"), (("--rows", "x"), "--rows"), (("--rows", "2"), "must exceed -c 2"),
                      (("--rows", "64", "-c", "64"), "must exceed -c 64")):
        r = subprocess.run([exe, "evaluate", "-s", cfg, "-K", "31", "--assembly", "x.fa", *opts, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opts}: {r.returncode} {r.stderr[:200]}"
    # the assembly file is not there; it holds no stretch of K letters: both before the library config is opened or the device is touched
    r = subprocess.run([exe, "evaluate", "-s", cfg, "-K", "31", "--assembly", str(tmp_path / "none.fa"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot read" in r.stderr
    short = tmp_path / "short.fa"
    short.write_text(">a\n" + "ACGTACGTAC" * 3 + "N" + "ACGTACGTAC" * 3 + "\n>b\nNNNN\n")
    r = subprocess.run([exe, "evaluate", "-s", cfg, "-K", "31", "--assembly", str(short), "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and "no stretch of 31 letters ACGT" in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
