"""CPU: the adapter and tail clipping exists at every layer (header, library, binding); the Python restatement of the rule
(read_clip_util.py) -- what the GPU tests expect -- against a second, independently written brute force over strings; the case of
tests/test_read_clip.py holds what it promises; the pure checks the stage adds to csrc/sdt_read_plan.h and the device-free half of
`sdt-kmers clip` (csrc/host/clipsplit.c) as stand-alone programs under AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np

import read_clip_util as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_clip_reads", "sdt_gpu_clip_reads_device", "sdt_gpu_clip_kept_reads"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_three_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    assert re.search(r"#define\s+SDT_CLIP_MAX_ADAPTERS\s+256\b", src) and re.search(r"#define\s+SDT_CLIP_MAX_ADAPTER_LEN\s+128\b", src)
    for words in ("base qualities", "indels", "IUPAC", "mate overlap", "reverse-complement", "inside pass 1", "251 were touched",
                  "they take an array of sdt_read_clip through a pointer cast"):
        assert words in src, f"include/sdt_gpu.h does not say {words!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+adapters,\s*tail3,\s*tail5,\s*start,\s*len,\s*verdict;\s*\}\s*sdt_read_clip;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+min_overlap,\s*max_err_pct,\s*min_len,\s*min_tail,\s*tail_err_pct,\s*tail3_bases,"
                     r"\s*tail5_bases,\s*flags;\s*\}\s*sdt_clip_params;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*const\s+uint32_t\s*\*words;\s*const\s+uint64_t\s*\*offsets;\s*const\s+uint8_t\s*\*ends;"
                     r"\s*uint32_t\s+n,\s*reserved;\s*\}\s*sdt_adapter_set;", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_read_clip_dtype_and_params_are_the_c_structs(pkg):
    import ctypes
    dt = pkg.READ_CLIP_DTYPE
    assert dt.itemsize == 24 and dt.names == rc.CLIP_FIELDS and dt == rc.CLIP_DTYPE
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20]
    # start, len and verdict sit where sdt_read_trim has them: compact_trimmed takes the records as they are
    for f in ("start", "len", "verdict"):
        assert dt.fields[f][1] == pkg.READ_TRIM_DTYPE.fields[f][1]
    assert dt.itemsize == pkg.READ_TRIM_DTYPE.itemsize
    assert ctypes.sizeof(pkg.ClipParams) == 32
    assert [(f, getattr(pkg.ClipParams, f).offset) for f, _ in pkg.ClipParams._fields_] == [(f, 4 * i) for i, f in enumerate(rc.PARAM_FIELDS)]
    assert ctypes.sizeof(pkg.AdapterSet) == 32 and pkg.AdapterSet.n.offset == 24 and pkg.AdapterSet.reserved.offset == 28
    assert (pkg.CLIP_WHOLE, pkg.CLIP_CLIPPED, pkg.CLIP_DROPPED) == (rc.WHOLE, rc.CLIPPED, rc.DROPPED) == (pkg.TRIM_WHOLE, pkg.TRIM_TRIMMED, pkg.TRIM_DROPPED)
    assert (pkg.CLIP_MAX_ADAPTERS, pkg.CLIP_MAX_ADAPTER_LEN) == (256, 128)
    for m in ("clip_reads", "clip_reads_device", "clip_kept_reads"):
        assert callable(getattr(pkg.PregraphGPU, m))
    # the packed set of the binding: 16 bases per word, the first in the most significant pair
    aset, (words, offsets, ends) = pkg.pack_adapters([([1, 2, 3, 0] * 5, 0), ([3] * 17, 1)])
    assert offsets.tolist() == [0, 20, 37] and ends.tolist() == [0, 1] and aset.n == 2
    assert words[:3].tolist() == [0x6C6C6C6C, 0x6CFFFFFF, 0xFFC00000] and (words[3:] == 0).all()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def brute_force(read, adapters, p):
    """the rule once more, over strings: every p, every e and every t is tried, none is skipped, and the best is picked from the list"""
    s = "".join("ACTG"[int(b)] for b in read)
    L = len(s)
    mism = lambda x, y: sum(a != b for a, b in zip(x, y))
    hits3, hits5 = [], []
    for i, (a, end) in enumerate(adapters):
        a = "".join("ACTG"[int(b)] for b in a)
        m = len(a)
        if end == 0:
            ok = [q for q in range(L) if min(m, L - q) >= p["min_overlap"]
                  and 100 * mism(s[q:q + min(m, L - q)], a[:min(m, L - q)]) <= p["max_err_pct"] * min(m, L - q)]
            if ok:
                hits3.append((min(ok), i))
        else:
            ok = [e for e in range(1, L + 1) if min(m, e) >= p["min_overlap"]
                  and 100 * mism(s[e - min(m, e):e], a[m - min(m, e):]) <= p["max_err_pct"] * min(m, e)]
            if ok:
                hits5.append((-max(ok), i))
    e0, a3 = min(hits3) if hits3 else (L, -1)             # the smallest p, the lowest index among equals
    s0, a5 = min(hits5) if hits5 else (0, -1)             # the largest e, the lowest index among equals
    s0 = -s0

    def tail_of(seg, letter):
        cand = []
        for t in range(1, len(seg) + 1):
            suffix = seg[len(seg) - t:]
            x = t - suffix.count(letter)
            if suffix[0] == letter and t >= p["min_tail"] and 100 * x <= p["tail_err_pct"] * t:
                cand.append((-(t - 3 * x), t))
        return min(cand)[1] if cand else 0

    t3 = t5 = 0
    if s0 < e0:
        t3 = max([tail_of(s[s0:e0], "ACTG"[b]) for b in range(4) if p["tail3_bases"] >> b & 1] + [0])
        t5 = max([tail_of(s[s0:e0 - t3][::-1], "ACTG"[b]) for b in range(4) if p["tail5_bases"] >> b & 1] + [0])
    start = s0 + t5
    ln = max(0, e0 - t3 - start)
    found = ((a3 + 1) | (a5 + 1) << 16, t3, t5)
    if ln < max(p["min_len"], 1):
        return found + (0, 0, rc.DROPPED), (s0, e0), (hits3, hits5)
    return found + (start, ln, rc.WHOLE if ln == L else rc.CLIPPED), (s0, e0), (hits3, hits5)


def test_restatement_equals_brute_force():
    """300 random reads of 0 .. 40 bases over two letters, adapters of 1 .. 6 bases: hits, ties and crossings abound"""
    rng = np.random.default_rng(7)
    verdicts, crossings, ties, tails = set(), 0, 0, 0
    for k in range(300):
        read = rng.integers(0, 2, size=int(rng.integers(0, 41)), dtype=np.uint8) * 2          # A and T
        mo = int(rng.integers(1, 4))
        adapters = [(rng.integers(0, 2, size=int(rng.integers(mo, 7)), dtype=np.uint8) * 2, int(rng.integers(0, 2)))
                    for _ in range(int(rng.integers(0, 5)))]
        p = rc.params(min_overlap=mo, max_err_pct=(0, 20, 34)[k % 3], min_len=int(rng.integers(0, 8)), min_tail=int(rng.integers(1, 5)),
                      tail_err_pct=(0, 20, 34)[(k // 3) % 3], tail3_bases=int(rng.integers(0, 16)), tail5_bases=int(rng.integers(0, 16)))
        want, (s0, e0), (hits3, hits5) = brute_force(read, adapters, p)
        got = rc.clip_read(read, adapters, p)
        assert got == want, f"read {k}: {read.tolist()} {[(a.tolist(), e) for a, e in adapters]} {p}: {got}, {want} by brute force"
        verdicts.add(want[5])
        crossings += s0 >= e0 and len(read) > 0
        ties += any(sum(h[0] == best for h in hits) > 1 for hits, best in ((hits3, e0), (hits5, -s0)) if hits)
        tails += want[1] > 0 or want[2] > 0
    assert verdicts == {rc.WHOLE, rc.CLIPPED, rc.DROPPED}
    assert crossings >= 1 and ties >= 1 and tails >= 10, (crossings, ties, tails)


def test_restatement_on_the_examples_of_the_rule():
    A, C, T, G = rc.A, rc.C, rc.T, rc.G
    p = rc.params(min_overlap=3, max_err_pct=10, min_tail=4, tail_err_pct=20, tail3_bases=1 << A, tail5_bases=1 << T)
    ad3, ad5 = ([C, G, C, G, G], 0), ([G, G, C, C, G], 1)
    body = [C, T, G, C, A, G, T, C]
    # a tail in front of a read-through adapter; the adapter continues past the read's end
    assert rc.clip_read(body + [A] * 5 + [C, G, C], [ad3], p) == (1, 5, 0, 0, 8, rc.CLIPPED)
    # the remnant of a 5' adapter, then a T head
    assert rc.clip_read([C, C, G] + [T] * 4 + body, [ad3, ad5], p) == (2 << 16, 0, 4, 7, 8, rc.CLIPPED)
    # two overlaps of 2 bases are too short
    assert rc.clip_read(body + [C, G], [ad3], p) == (0, 0, 0, 0, 10, rc.WHOLE)
    # a tie in score goes to the shorter tail: AAAA (4) against AAAA C AA (7 - 3 = 4)
    assert rc.clip_read(body + [A, A, C, A, A, A, A], [], p) == (0, 4, 0, 0, 11, rc.CLIPPED)
    # the lowest index wins among adapters that hit at the same p
    assert rc.clip_read(body + [C, G, C, G], [([C, G, C], 0), ad3], p)[0] == 1
    assert rc.clip_read(body + [C, G, C, G], [ad3, ([C, G, C], 0)], p)[0] == 1
    # min_len; a dropped read's record still says what was found
    assert rc.clip_read(body + [C, G, C], [ad3], dict(p, min_len=9)) == (1, 0, 0, 0, 0, rc.DROPPED)
    assert rc.clip_read([], [ad3], p) == (0, 0, 0, 0, 0, rc.DROPPED)


def test_the_case_holds_what_it_says():
    c = rc.case()
    assert 100 <= len(c["reads"]) <= 140 and rc.case_holds() >= 35
    lens = sorted(len(a) for a, _ in c["adapters"])
    assert {31, 32, 33, 64, 65, 128} <= set(lens) and {e for _, e in c["adapters"]} == {0, 1}
    assert max(len(r) for r in c["reads"]) == 5000
    # reads start at every base of a word
    assert len({int(o) & 15 for o in c["offs"][:-1]}) == 16
    # the texts of the command line tool on the case, by hand on its smallest part
    names = [f"ad{i}" for i in range(len(c["adapters"]))]
    clip = rc.case_expect()[0]
    rec, pairs, single, stats = rc.cli_texts(c["codes"], c["offs"], clip, [], names, [e for _, e in c["adapters"]])
    assert rec.count("\n") == len(c["reads"]) and pairs == "" and single.count(">") == int((clip["len"] > 0).sum())
    lines = stats.splitlines()
    assert len(lines) == len(names) + 5 and lines[-3:] == [f"whole {(clip['verdict'] == 0).sum()}", f"clipped {(clip['verdict'] == 2).sum()}",
                                                          f"dropped {(clip['verdict'] == 3).sum()}"]


# ---- the pure checks of csrc/sdt_read_plan.h --------------------------------------------------------------------------------------------
def test_parameter_and_adapter_checks_clean_under_sanitizers(tmp_path):
    """tools/clip_plan_check.cpp: every refusal of the parameters and of the adapter set, the boundaries 128 / 129 bases and 256 / 257
    adapters, the split of an adapter into chunks; includes sdt_read_plan.h alone"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "clip_plan_check.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["../soapdenovo-trans_amd/csrc/sdt_read_plan.h"]
    exe = str(tmp_path / "clip_plan_check")
    subprocess.run([cxx, "-std=c++17"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("clip_plan_check: ok"), r.stdout + r.stderr


# ---- the device-free half of `sdt-kmers clip` -----------------------------------------------------------------------------------------
def test_adapter_files_record_line_and_stats_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "clip_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "clip_host_check.c"), os.path.join(host, "clipsplit.c")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "clip_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_sdt_kmers_usage_knows_clip(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    for args in ((), ("clip",), ("clip", "-s", "lib.cfg")):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 255
        for word in ("sdt-kmers clip -s lib.cfg -K k", "-a adapters3.fa", "-g adapters5.fa", "--tail3", "--tail5", "--min-overlap N, default 5",
                     "--error-pct P, default 10", "--min-tail N, default 10", "--tail-error-pct P, default 20", "--min-len L, default 0",
                     "prefix.readClip", "prefix.clip.pairs.fa", "prefix.clip.single.fa", "prefix.clipStats",
                     "adapter3 adapter5 tail3 tail5 start len verdict"):
            assert word in r.stderr, f"sdt-kmers {' '.join(args)}: the usage text lacks {word!r}"
    cfg = str(tmp_path / "none.cfg")                    # (never opened: the options are refused first)
    out = str(tmp_path / "out")
    for sub in ("profile", "correct", "normalize", "trim", "dedup", "query"):
        for opt in (("-a", "x.fa"), ("-g", "x.fa"), ("--tail3", "A"), ("--tail5", "T"), ("--min-overlap", "5"), ("--error-pct", "10"),
                    ("--min-tail", "10"), ("--tail-error-pct", "20")):
            r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
            assert r.returncode == 255 and f"{opt[0]} belongs to clip" in r.stderr, f"{sub} {opt}: {r.returncode} {r.stderr[:200]}"
    for opt, bad, say in (("--error-pct", "101", "whole number"), ("--tail-error-pct", "x", "whole number"), ("--min-overlap", "0", "at least 1"),
                          ("--min-tail", "0", "at least 1"), ("--tail3", "AN", "letters of ACGT"), ("--min-len", "-1", "whole number")):
        r = subprocess.run([exe, "clip", "-s", cfg, "-K", "31", opt, bad, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and opt in r.stderr and say in r.stderr, f"{opt} {bad}: {r.returncode} {r.stderr[:200]}"
    r = subprocess.run([exe, "clip", "-s", cfg, "-K", "31", "--mate-swap", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and "--mate-swap belongs to dedup" in r.stderr
    # an adapter file with a letter that is no base: refused with the file and the line before the library config is opened
    bad = tmp_path / "bad.fa"
    bad.write_text(">one\nACGT\n>two\nACGNT\n")
    r = subprocess.run([exe, "clip", "-s", cfg, "-K", "31", "-a", str(bad), "-o", out], capture_output=True, text=True)
    assert r.returncode == 2 and f"{bad} line 4: 'N' is not one of ACGT" in r.stderr
    short = tmp_path / "short.fa"
    short.write_text(">tiny\nACG\n")
    r = subprocess.run([exe, "clip", "-s", cfg, "-K", "31", "-g", str(short), "-o", out], capture_output=True, text=True)
    assert r.returncode == 2 and "tiny" in r.stderr and "--min-overlap" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
