"""The correction rule of include/sdt_gpu.h (sdt_gpu_correct_reads) restated in plain Python: what the tests of the kernel, the ABI
and `sdt-kmers correct` expect.  A table is anything with .get(canonical k-mer as an integer, 0) -> count; nothing here touches the
library under test."""
import numpy as np

from test_kmer_search import canon_kmers

FIX_FIELDS = ("kmers", "weak", "runs", "fixed")
LETTERS = "ACTG"


def runs_of(weak):
    """maximal stretches [a, b] of True"""
    out = []
    a = None
    for j, w in enumerate(weak):
        if w and a is None:
            a = j
        if not w and a is not None:
            out.append((a, j - 1))
            a = None
    if a is not None:
        out.append((a, len(weak) - 1))
    return out


def candidate_base(a, b, n, K):
    """the base a run [a, b] of a read with n k-mers points at, or None"""
    l = b - a + 1
    if a == 0 and b == n - 1:
        return None
    if a > 0 and b < n - 1:
        return b if l == K else None
    if l > K:
        return None
    return b if a == 0 else a + K - 1


def correct_read(codes, K, count, min_count, kmer_counts=None):
    """codes: uint8 bases of one read; count(canonical k-mer) -> count; kmer_counts: the counts of the read's k-mers, if the caller has
    them.  -> ((kmers, weak, runs, fixed), [(pos, new_base)] ascending)"""
    n = len(codes) - K + 1
    if n <= 0:
        return (0, 0, 0, 0), []
    c = kmer_counts if kmer_counts is not None else [count(k) for k in canon_kmers(codes, K)]
    weak = [x < min_count for x in c]
    nweak = sum(weak)
    if not nweak:
        return (n, 0, 0, 0), []
    runs = runs_of(weak)
    subs = []
    for a, b in runs:
        p = candidate_base(a, b, n, K)
        if p is None:
            continue
        window = codes[a:b + K].copy()                   # the bases of k-mers a .. b, judged on the read as it came
        valid = []
        for x in range(4):
            if x == codes[p]:
                continue
            window[p - a] = x
            if all(count(k) >= min_count for k in canon_kmers(window, K)):
                valid.append(x)
        if len(valid) == 1:
            subs.append((p, valid[0]))
    return (n, nweak, len(runs), len(subs)), subs


def table_counts(nodes):
    """the oracle's node dictionary (test_kmer_search.node_dict_oracle: key -> (l, r, count)) or a Counter -> count(k)"""
    def count(k):
        v = nodes.get(k, 0)
        return v[2] if isinstance(v, tuple) else v
    return count


def read_kmer_counts(codes, offs, K, count):
    """the counts of every read's k-mers, once per table: they do not depend on min_count"""
    return [[count(k) for k in canon_kmers(codes[int(offs[r]):int(offs[r + 1])], K)] for r in range(len(offs) - 1)]


def expect_correct(codes, offs, K, count, min_count, kmer_counts=None, ordinals=None):
    """-> (fix records as a structured array, the corrected codes, the edits uint64 ascending: read << 18 | pos << 2 | new_base with
    read = the index in the batch, or ordinals[index])"""
    n = len(offs) - 1
    fix = np.zeros(n, dtype=[(f, np.uint32) for f in FIX_FIELDS])
    out = codes.copy()
    edits = []
    for r in range(n):
        s, e = int(offs[r]), int(offs[r + 1])
        rec, subs = correct_read(codes[s:e], K, count, min_count, None if kmer_counts is None else kmer_counts[r])
        fix[r] = rec
        for p, x in subs:
            out[s + p] = x
            edits.append((int(ordinals[r]) if ordinals is not None else r) << 18 | p << 2 | x)
    return fix, out, np.array(sorted(edits), dtype=np.uint64)


def assert_fix_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names == FIX_FIELDS
    for f in FIX_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


def cli_texts(codes, offs, fix, out, edits):
    """the three files of `sdt-kmers correct` for a stream in ordinal order"""
    fix_txt = "".join(f"{a} {b} {c} {d}\n" for a, b, c, d in fix.tolist())
    ed = []
    for e in edits.tolist():
        r, p, x = e >> 18, (e >> 2) & 0xFFFF, e & 3
        ed.append(f"{r + 1} {p + 1} {LETTERS[codes[int(offs[r]) + p]]} {LETTERS[x]}\n")
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)[out].tobytes().decode()
    fa = "".join(f">{r + 1}\n{letters[int(offs[r]):int(offs[r + 1])]}\n" for r in range(len(offs) - 1))
    return fix_txt, "".join(ed), fa
