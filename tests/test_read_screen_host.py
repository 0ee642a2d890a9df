"""CPU: the reference screen exists at every layer (header, library, binding); the Python restatement of the rule (read_screen_util.py) --
what the GPU tests expect -- on examples worked by hand and against a second restatement over strings; the named cases hold what they
promise; the pure functions the stage adds to csrc/sdt_read_plan.h and the device-free half of `sdt-kmers screen`
(csrc/host/screensplit.c) as stand-alone programs under AddressSanitizer + UBSan; the refusals of the command line that need no
device."""
import os
import re
import shutil
import subprocess

import numpy as np

import read_screen_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_screen_load", "sdt_gpu_screen_unload", "sdt_gpu_screen_info", "sdt_gpu_screen_lookup", "sdt_gpu_screen_reads",
           "sdt_gpu_screen_reads_device", "sdt_gpu_screen_kept_reads"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_seven_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    for words in ("the smaller of itself and its reverse complement", "11 <= k <= 31", "the SMALLEST ref_of_seq", "references listed first win",
                  "kmers = max(L - k + 1, 0)", "hits >= max(min_hits, 1) and 100 hits >= min_hit_pct kmers", "A unit is matched iff one of its",
                  "SDT_SCREEN_KEEP_MATCHED: an unmatched unit is dropped", "start = 0, len = L if kept, else 0", "only once the new one is complete",
                  "a set without a single k-mer", "NO limit on the read length in any form", "16 B per slot", "Hamming-distance or IUPAC matching",
                  "masking the matching bases", "majority", "k above 31", "sets larger than device memory", "any change to another stage",
                  "An N inside a read is a G in the stream", "a choice, not a measurement", "a pair with one", "has NO length limit"):
        assert words in src, f"include/sdt_gpu.h does not say {words!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+kmers,\s*hits,\s*ref,\s*start,\s*len,\s*verdict;\s*\}\s*sdt_read_screen;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+min_hits,\s*min_hit_pct,\s*flags,\s*reserved;\s*\}\s*sdt_screen_params;", src)
    assert re.search(r"#define\s+SDT_SCREEN_KEEP_MATCHED\s+1u", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_read_screen_dtype_and_params_are_the_c_structs(pkg):
    import ctypes
    dt = pkg.READ_SCREEN_DTYPE
    assert dt.itemsize == 24 and dt.names == su.FIELDS and dt == su.DTYPE
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20]
    # start, len and verdict sit where sdt_read_trim has them: compact_trimmed takes the records as they are
    for f in ("start", "len", "verdict"):
        assert dt.fields[f][1] == pkg.READ_TRIM_DTYPE.fields[f][1]
    assert dt.itemsize == pkg.READ_TRIM_DTYPE.itemsize
    assert ctypes.sizeof(pkg.ScreenParams) == 16
    fields = ("min_hits", "min_hit_pct", "flags", "reserved")
    assert [(f, getattr(pkg.ScreenParams, f).offset) for f, _ in pkg.ScreenParams._fields_] == [(f, 4 * i) for i, f in enumerate(fields)]
    d = pkg.ScreenParams()
    assert {f: getattr(d, f) for f in fields} == su.params()                  # the defaults of the command line
    assert pkg.SCREEN_KEEP_MATCHED == su.KEEP_MATCHED == 1 and pkg.SCREEN_NO_REF == su.NO_REF and (pkg.SCREEN_KEPT, pkg.SCREEN_DROPPED) == (su.KEPT, su.DROPPED)
    for m in ("screen_load", "screen_unload", "screen_info", "screen_lookup", "screen_reads", "screen_reads_device", "screen_kept_reads"):
        assert callable(getattr(pkg.PregraphGPU, m))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
RANK = {"A": 0, "C": 1, "T": 2, "G": 3}                                       # the stream's codes order the k-mers


def by_strings(seq_texts, refs, read_text, k):
    """the rule once more, over strings: every k-mer and its reverse complement as text, the smaller by the stream's codes"""
    key = lambda s: [RANK[c] for c in s]
    canon = lambda s: min(s, "".join(COMP[c] for c in reversed(s)), key=key)
    table = {}
    for text, r in zip(seq_texts, refs):
        for i in range(len(text) - k + 1):
            x = canon(text[i:i + k])
            table[x] = min(table.get(x, su.NO_REF), r)
    found = [table[canon(read_text[i:i + k])] for i in range(len(read_text) - k + 1) if canon(read_text[i:i + k]) in table]
    return max(len(read_text) - k + 1, 0), len(found), min(found) if found else su.NO_REF


def test_restatement_equals_the_second_restatement():
    rng = np.random.default_rng(9)
    text = lambda codes: "".join(su.LETTERS[int(c)] for c in codes)
    for k in (11, 12, 16, 31):
        seqs = [rng.integers(0, 4, size=int(n), dtype=np.uint8) for n in rng.integers(0, 300, size=12)]
        seqs[3] = su.revcomp(seqs[1])[20:]                                     # a reference that is another one's reverse strand
        refs = [int(r) for r in rng.integers(0, 4, size=12)]
        d = su.build_set(seqs, refs, k)
        hits = 0
        for i in range(60):
            src = seqs[i % 12]
            cut = src[len(src) // 3:len(src) // 3 + int(rng.integers(0, 120))]
            read = np.concatenate([cut if i % 3 else su.revcomp(cut), rng.integers(0, 4, size=int(rng.integers(0, 40)), dtype=np.uint8)]).astype(np.uint8)
            want = by_strings([text(s) for s in seqs], refs, text(read), k)
            assert su.read_facts(read, k, d) == want, (k, i)
            hits += want[1] > 0
        assert hits >= 30


def test_restatement_on_examples_by_hand():
    a = lambda s: np.array([su.LETTERS.index(c) for c in s], dtype=np.uint8)
    # canonical forms: A < C < T < G as integers; AAAAAAAAAAA (0) is its own smaller strand, TTTTTTTTTTT is stored as it
    assert su.canonical_kmers(a("T" * 11), 11) == [0] and su.canonical_kmers(a("A" * 12), 11) == [0, 0]
    assert su.revcomp_int(su.kmer_int(a("ACGTTGCAAGC")), 11) == su.kmer_int(a("GCTTGCAACGT"))
    pal = a("ACGTTGCAGCTGCAACGT"[:8])
    pal = np.concatenate([pal, su.revcomp(pal)])
    assert su.revcomp_int(su.kmer_int(pal), 16) == su.kmer_int(pal)            # a palindrome of even k is its own reverse complement
    # X has 3 k-mers; Y is a G in front of the reverse complement of X's first k-mer: 2 k-mers, one of them X's first on the other strand
    X = a("AACCTTGGACTGA")
    Y = np.concatenate([a("G"), su.revcomp(X[:11])])
    d = su.build_set([X, Y, a("AACCTTGGAC")], [2, 1, 0], 11)
    # the third sequence (k - 1 bases) contributes nothing; the shared k-mer goes to the smaller reference whatever the order
    first = su.canonical_kmers(X, 11)[0]
    assert len(d) == 4 and sorted(d.values()) == [1, 1, 2, 2] and d[first] == 1 and su.build_set([Y, X], [1, 2], 11) == d
    assert su.read_facts(X, 11, d) == (3, 3, 1) and su.read_facts(su.revcomp(X), 11, d) == (3, 3, 1) and su.read_facts(X[1:], 11, d) == (2, 2, 2)
    assert su.read_facts(a("AACCTTGGAC"), 11, d) == (0, 0, su.NO_REF) and su.read_facts(a(""), 11, d) == (0, 0, su.NO_REF)
    # the rule of a read at its boundaries
    assert su.read_matched(100, 1, su.params()) and not su.read_matched(100, 0, su.params(min_hits=0)) and su.read_matched(100, 1, su.params(min_hits=0))
    assert su.read_matched(100, 37, su.params(min_hit_pct=37)) and not su.read_matched(100, 36, su.params(min_hit_pct=37)) and not su.read_matched(0, 0, su.params(min_hit_pct=0))
    # units and flags
    facts = [(80, 80, 0), (80, 0, su.NO_REF), (80, 0, su.NO_REF), (80, 0, su.NO_REF)]
    rec, keep, kept = su.verdicts(facts, [100] * 4, su.params(), su.dense_units(4, True))
    assert rec["verdict"].tolist() == [1, 1, 0, 0] and rec["len"].tolist() == [0, 0, 100, 100] and rec["hits"].tolist() == [80, 0, 0, 0] and kept == 2
    rec, keep, kept = su.verdicts(facts, [100] * 4, su.params(flags=su.KEEP_MATCHED), su.dense_units(4, False))
    assert rec["verdict"].tolist() == [0, 1, 1, 1] and keep.tolist() == [1, 0, 0, 0]
    assert su.ranged_units([3, 4, 5, 7, 9], [(3, 7)]) == [[3, 4], [5], [7], [9]]


def test_the_cases_hold_what_they_say():
    for k in su.KS:
        c, d, rc = su.set_case(k), su.set_dict(k), su.read_case(k)
        lens = sorted(len(s) for s in c["seqs"])
        assert lens[-1] == 20000 and 6000 in lens and {0, 3, k - 1, k, k + 1} <= set(lens) and len(set(c["refs"])) == su.N_REFS
        assert su.positions(c["seqs"], k) == su.SET_POSITIONS and 0.9 * 32768 < len(d) <= su.SET_POSITIONS
        assert {len(r) for r in rc["reads"]} >= {0, k - 1, k, k + 1, k + 63, k + 64, 200, 5000}
        kinds = [(f[0], f[1]) for f in rc["facts"]]
        assert any(h == n > 0 for n, h in kinds) and any(h == 0 < n for n, h in kinds) and any(0 < h < n for n, h in kinds)
    # the texts of the command line on two reads by hand
    rec = np.array([(5, 5, 1, 0, 0, 1), (0, 0, su.NO_REF, 0, 3, 0)], dtype=su.DTYPE)
    codes = np.array([0] * 15 + [1, 2, 3], dtype=np.uint8)
    texts = su.cli_texts(codes, np.array([0, 15, 18], dtype=np.uint64), rec, [], ["x", "y"], [10, 20], su.params())
    assert texts == ("5 5 2 1\n0 0 0 0\n", "", ">2\nCTG\n", "1 x 10 0 0\n2 y 20 1 5\n# reads 2 matched 1 kept 1 dropped 1\n")
    assert su.parse_refs([">a b\nACGTNNac\ngt\n\n>n\nNNN\n", ">c\nAC\n"])[1:] == ([0, 0, 2], ["a", "n", "c"], [8, 0, 2])


# ---- the pure functions of csrc/sdt_read_plan.h -----------------------------------------------------------------------------------------
def test_parameter_check_and_unit_verdicts_clean_under_sanitizers(tmp_path):
    """tools/screen_plan_check.cpp: every refusal, the table sizes, the rule of a read, and the unit verdicts of the kept form against a
    walk over every ordinal on random ranges; includes sdt_read_plan.h alone"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "screen_plan_check.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["../soapdenovo-trans_amd/csrc/sdt_read_plan.h"]
    exe = str(tmp_path / "screen_plan_check")
    subprocess.run([cxx, "-std=c++17"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("screen_plan_check: ok"), r.stdout + r.stderr


# ---- the device-free half of `sdt-kmers screen` -----------------------------------------------------------------------------------------
def test_fasta_reader_record_line_and_statistics_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "screen_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "screen_host_check.c"), os.path.join(host, "screensplit.c")],
                   check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "screen_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_sdt_kmers_usage_knows_screen(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    for args in ((), ("screen",), ("screen", "-s", "lib.cfg")):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 255
        for word in ("sdt-kmers screen -s lib.cfg -K k", "-r refs.fa [-r more.fa ...]", "--screen-k S, default 31", "--min-hits N, default 1",
                     "--min-hit-pct P, default 0", "--keep-matched", "prefix.readScreen", "prefix.screen.pairs.fa", "prefix.screen.single.fa",
                     "prefix.screenStats", "kmers hits ref verdict", "index name\n              bases reads hits", "# reads R matched M kept K dropped D",
                     "usual figure of bbduk: a choice, not a measurement", "An N in a read is a G"):
            assert word in r.stderr, f"sdt-kmers {' '.join(args)}: the usage text lacks {word!r}"
    cfg = str(tmp_path / "none.cfg")                    # (never opened: the options are refused first)
    out = str(tmp_path / "out")
    for sub in ("profile", "correct", "normalize", "trim", "dedup", "clip", "overlap", "complexity", "qtrim", "query"):
        for opt in (("-r", "x.fa"), ("--screen-k", "21"), ("--min-hits", "2"), ("--min-hit-pct", "5"), ("--keep-matched",)):
            r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
            assert r.returncode == 255 and f"{opt[0]} belongs to screen" in r.stderr, f"{sub} {opt}: {r.returncode} {r.stderr[:200]}"
    for opt, say in ((("-a", "x.fa"), "-a belongs to clip"), (("--max-score", "5"), "--max-score belongs to complexity"), (("--mate-swap",), "--mate-swap belongs to dedup"),
                     (("--target", "5"), "--target belongs to normalize"), (("--min-len", "5"), "--min-len belongs to trim"), (("--cut-q", "5"), "--cut-q belongs to qtrim")):
        r = subprocess.run([exe, "screen", "-s", cfg, "-K", "31", "-r", "x.fa", *opt, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opt}: {r.returncode} {r.stderr[:200]}"
    for opts, say in ((("--screen-k", "10"), "--screen-k"), (("--screen-k", "32"), "--screen-k"), (("--screen-k", "x"), "--screen-k"),
                      (("--min-hit-pct", "101"), "--min-hit-pct"), (("--min-hits", "-1"), "--min-hits"), (("--min-hits", "1e3"), "--min-hits")):
        r = subprocess.run([exe, "screen", "-s", cfg, "-K", "31", "-r", "x.fa", *opts, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opts}: {r.returncode} {r.stderr[:200]}"
    # no reference file at all
    r = subprocess.run([exe, "screen", "-s", cfg, "-K", "31", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and "-r refs.fa" in r.stderr
    # the options are fine, the reference file is not there: refused before the library config is opened or the device is touched
    r = subprocess.run([exe, "screen", "-s", cfg, "-K", "31", "-r", str(tmp_path / "none.fa"), "--screen-k", "11", "--min-hits", "0", "--min-hit-pct", "100",
                        "--keep-matched", "-o", out], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot read" in r.stderr and "belongs to" not in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
