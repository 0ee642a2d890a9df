"""The rule of the table comparison (include/sdt_gpu.h: sdt_gpu_compare_tables, sdt_gpu_compare_select) restated in plain Python -- what
the GPU tests and the command-line test expect -- and the case they run.  A table is a dict canonical k-mer -> count from the oracle
(asm_support_util.oracle_counts), never from the library under test; matrix, totals, selection and the texts of `sdt-kmers compare`
are plain loops.  All comparisons against it are exact."""
import functools

import numpy as np

import asm_support_util as au

MAX_CELLS = 16384
U32 = 2**32 - 1


def compare(A, B, rows, cols):
    """-> (matrix uint64[rows, cols], totals uint64[8]) of two tables"""
    m = np.zeros((rows, cols), dtype=np.uint64)
    t = [0] * 8
    for k in set(A) | set(B):
        ca, cb = A.get(k, 0), B.get(k, 0)
        m[min(ca, rows - 1), min(cb, cols - 1)] += 1
        if k in A:
            t[0] += 1
            t[3] += ca
        if k in B:
            t[1] += 1
            t[4] += cb
        if k in A and k in B:
            t[2] += 1
            t[5] += min(ca, cb)
            t[6] += ca
            t[7] += cb
    return m, np.array(t, dtype=np.uint64)


def select(A, B, min_a=1, max_a=U32, min_b=0, max_b=0):
    """-> {(k-mer, cA, cB)}: the k-mers IN A within both ranges; cB = 0 for a k-mer that is not in B"""
    return {(k, ca, B.get(k, 0)) for k, ca in A.items() if min_a <= ca <= max_a and min_b <= B.get(k, 0) <= max_b}


def swapped(totals):
    t = [int(x) for x in totals]
    return np.array([t[1], t[0], t[2], t[4], t[3], t[5], t[7], t[6]], dtype=np.uint64)


def key_ints(keys):
    """rows of key words, most significant first -> Python integers"""
    out = []
    keys = np.asarray(keys, dtype=np.uint64)
    for row in (keys.reshape(len(keys), -1).tolist() if keys.size else []):
        v = 0
        for x in row:
            v = (v << 64) | int(x)
        out.append(v)
    return out


def records(keys, ca, cb):
    """what compare_select gave, as the set select() gives"""
    rec = list(zip(key_ints(keys), (int(x) for x in ca), (int(x) for x in cb)))
    assert len(set(rec)) == len(rec), "a k-mer was listed twice"
    return set(rec)


# ---- the texts of `sdt-kmers compare` -------------------------------------------------------------------------------------------------------
def kmer_text(k, K):
    return "".join(au.LETTERS[(k >> (2 * (K - 1 - i))) & 3] for i in range(K))


def matrix_text(m):
    rows, cols = m.shape
    head = "a\\b " + " ".join(str(c) + ("+" if c == cols - 1 else "") for c in range(cols)) + "\n"
    return head + "".join(str(r) + ("+ " if r == rows - 1 else " ") + " ".join(str(int(x)) for x in m[r]) + "\n" for r in range(rows))


def kmers_text(sel, K, max_list=None):
    """the whole selection ascending by key; with max_list below its size only the last line is determined"""
    lines = [f"{kmer_text(k, K)} {ca} {cb}\n" for k, ca, cb in sorted(sel)]
    if max_list is not None and len(lines) > max_list:
        return None, f"# {len(lines)} matched\n"
    return "".join(lines), None


def summary_fields(totals, m, min_count):
    """(X, Y, S, P, Q, T, J, U, V, W), all integers: floors, and 0 where the divisor is 0"""
    t = [int(x) for x in totals]
    X, Y, S = t[0], t[1], t[2]
    P, Q, T = int(m[min_count:].sum()), int(m[:, min_count:].sum()), int(m[min_count:, min_count:].sum())
    div = lambda a, b: 10000 * a // b if b else 0
    return X, Y, S, P, Q, T, div(S, X + Y - S), div(S, X), div(S, Y), div(t[3] + t[4] - 2 * t[5], t[3] + t[4])


def summary_text(totals, m, min_count):
    return ("compare: nodes_a %d nodes_b %d shared %d solid_a %d solid_b %d solid_shared %d jaccard_x10000 %d contain_a_x10000 %d "
            "contain_b_x10000 %d braycurtis_x10000 %d\n" % summary_fields(totals, m, min_count))


# ---- the case ---------------------------------------------------------------------------------------------------------------------------------
HOT_A, HOT_B = 300, 320                                 # poly-A reads of K + 250 bases: 251 occurrences each, 75 300 and 80 320 in all


@functools.lru_cache(maxsize=None)
def pair_case(synth, K):
    """Two libraries per K.  A: 1 500 reads of K + 110 bases from 8 short transcripts (asm_support_util._reads).  B: 1 500 reads from 8
    transcripts of which the first 4 are A's, under another seed and another expression, and 4 are new.  Both hold poly-A reads of
    K + 250 bases, 300 in A and 320 in B: one shared node is counted past 65 535 on each side, differently.  The read length carries
    that for every K the library takes (251 k-mers per read whatever K is), so no K is reduced.
    -> dict: K, a / b (codes, offs), A / B (tables), kmers_a / nodes_a / kmers_b / nodes_b, polya"""
    L, hot_len = K + 110, K + 250
    tx, (acodes, aoffs) = au._reads(synth, K, 8, 1500, L, (HOT_A, hot_len), seed=200 + K, lo=300, hi=700)
    codes, starts, _ = tx
    ncodes, nstarts, _ = synth.make_transcriptome(4, seed=300 + K, lo=300, hi=700)
    bcodes = np.concatenate([codes[:int(starts[4])], ncodes])
    bstarts = np.concatenate([starts[:5], int(starts[4]) + nstarts[1:]]).astype(np.int64)
    rng = np.random.default_rng(400 + K)
    w = rng.lognormal(0.0, 2.0, size=8) * (bstarts[1:] - bstarts[:-1])
    rcodes, roffs = synth.sample_reads(bcodes, bstarts, w / w.sum(), n_reads=1500, read_len=L, seed=401 + K, err=0.002)
    reads = [rcodes[int(roffs[i]):int(roffs[i + 1])] for i in range(len(roffs) - 1)] + [np.zeros(hot_len, dtype=np.uint8)] * HOT_B
    bcodes_r, boffs = au.concat(reads)
    A, kmers_a, nodes_a = au.oracle_counts(acodes, aoffs, K)
    B, kmers_b, nodes_b = au.oracle_counts(bcodes_r, boffs, K)
    polya = au.canon_kmers(np.zeros(K, dtype=np.uint8), K)[0]
    case = {"K": K, "a": (acodes, aoffs), "b": (bcodes_r, boffs), "A": A, "B": B, "kmers_a": kmers_a, "nodes_a": nodes_a, "kmers_b": kmers_b,
            "nodes_b": nodes_b, "polya": polya}
    # what the GPU tests rely on: a degenerate fixture fails here, on the CPU
    m, t = compare(A, B, 64, 64)
    assert len(A) == nodes_a and len(B) == nodes_b
    assert t[2] > 100 and t[0] - t[2] > 100 and t[1] - t[2] > 100, "shared, A-only and B-only nodes"
    assert m[63, :63].sum() >= 1 and m[:63, 63].sum() >= 1 and m[63, 63] >= 1, "cells in the cap row, in the cap column and in both"
    assert m[1:, 0].sum() >= 1 and m[0, 1:].sum() >= 1 and m[0, 0] == 0 and m[1:63, 1:63].sum() >= 1
    assert A[polya] == HOT_A * 251 > 65535 and B[polya] == HOT_B * 251 > 65535 and A[polya] != B[polya], "one shared node past 65 535 on both sides"
    assert sum(c > 65535 for c in A.values()) == 1 and sum(c > 65535 for c in B.values()) == 1
    assert len(select(A, B, 0, U32, 0, U32)) == nodes_a > 2 * 256 * 8, "the selection of everything closes chunks in every wavefront of two workgroups"
    return case
