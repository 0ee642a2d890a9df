"""The rule of the assembly evaluation (include/sdt_gpu.h: sdt_gpu_asm_*) restated in plain Python -- what the GPU tests and the command-line
test expect -- and the cases they run.  Counts come from the oracle (a dict canonical k-mer -> count), never from the library under
test; records, the copy-number tally and the spectrum are plain loops.  All comparisons against it are exact."""
import functools
import math

import numpy as np

LETTERS = "ACTG"                                      # the stream's codes: A 0, C 1, T 2, G 3; complement = code ^ 2
FIELDS = ("sum", "kmers", "found", "solid", "gaps", "longest_gap", "longest_at")
DTYPE = np.dtype([("sum", np.uint64)] + [(f, np.uint32) for f in FIELDS[1:]])
CN_COLS, CN_MAX, MAX_ROWS = 8, 255, 1024


def codes_of(text):
    return np.array([LETTERS.index(c) for c in text.upper()], dtype=np.uint8)


def text_of(codes):
    return "".join(LETTERS[int(c)] for c in codes)


def revcomp(codes):
    return (codes[::-1] ^ 2).astype(np.uint8)


def canon_kmers(codes, K):
    """the canonical k-mers of a sequence as integers, first base most significant"""
    mask, top = (1 << (2 * K)) - 1, 2 * (K - 1)
    fw = rc = 0
    out = []
    for i, c in enumerate(np.asarray(codes).tolist()):
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((c ^ 2) << top)
        if i >= K - 1:
            out.append(fw if fw < rc else rc)
    return out


def concat(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    codes = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if seqs else np.zeros(0, dtype=np.uint8)
    return codes.astype(np.uint8), offs


def oracle_counts(codes, offs, K):
    """canonical k-mer -> count, from the oracle's table after pass 1 over the reads"""
    import oracle_binding as ob
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    keys, _, _, cnt, _ = o.export()
    out = {}
    for row, c in zip(keys.tolist(), cnt.tolist()):
        v = 0
        for x in row:
            v = (v << 64) | int(x)
        out[v] = int(c)
    return out, o.kmers_in_reads(), o.node_count()


def seq_record(ks, counts, min_count):
    """the record of one sequence from its canonical k-mers: (sum, kmers, found, solid, gaps, longest_gap, longest_at)"""
    mc = max(min_count, 1)
    n = len(ks)
    total = found = solid = gaps = best = run = start = 0
    best_at = n
    for j, k in enumerate(ks):
        c = counts.get(k, 0)
        total += c
        found += k in counts
        if c < mc:
            if run == 0:
                gaps += 1
                start = j
            run += 1
            if run > best:                            # (strictly: the first among equals stays)
                best, best_at = run, start
        else:
            solid += 1
            run = 0
    return (total, n, found, solid, gaps, best, best_at)


def support(seqs, K, counts, min_count, cn=None):
    """records of the sequences, and the tally node -> min(occurrences, 255) (added to cn if given)"""
    cn = {} if cn is None else cn
    rec = np.zeros(len(seqs), dtype=DTYPE)
    for i, s in enumerate(seqs):
        ks = canon_kmers(s, K)
        rec[i] = seq_record(ks, counts, min_count)
        for k in ks:
            if k in counts:
                cn[k] = min(cn.get(k, 0) + 1, CN_MAX)
    return rec, cn


def spectrum(counts, cn, rows):
    m = np.zeros((rows, CN_COLS), dtype=np.uint64)
    for k, c in counts.items():
        m[min(c, rows - 1), min(cn.get(k, 0), CN_COLS - 1)] += 1
    return m


def totals(rec):
    return np.array([len(rec), rec["kmers"].sum(), rec["found"].sum(), rec["solid"].sum()], dtype=np.uint64)


def assert_records_equal(got, want, what=""):
    assert got.dtype == DTYPE and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at sequences {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


def gaps_of(ks, counts, min_count):
    """[(first k-mer, length)] of the gaps of a sequence"""
    mc = max(min_count, 1)
    out = []
    for j, k in enumerate(ks):
        if counts.get(k, 0) < mc:
            if out and out[-1][0] + out[-1][1] == j:
                out[-1] = (out[-1][0], out[-1][1] + 1)
            else:
                out.append((j, 1))
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def substituted(seq, at):
    s = np.array(seq, dtype=np.uint8)
    s[at] = (s[at] + 1) & 3
    return s


def _reads(synth, K, T, n_reads, L, hot, seed, lo=500, hi=4000):
    tx = synth.make_transcriptome(T, seed=seed, lo=lo, hi=hi)
    codes, offs = synth.sample_reads(*tx, n_reads=n_reads, read_len=L, seed=seed + 1, err=0.002)
    reads = [codes[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)] + [np.zeros(hot[1], dtype=np.uint8)] * hot[0]
    return tx, concat(reads)


NAMED_K, NAMED_ROWS, NAMED_MIN_COUNT = 31, 64, 2


@functools.lru_cache(maxsize=None)
def named_case(synth):
    """the named case of the evaluation at K = 31: reads of a transcriptome of 40 plus 600 poly-A reads of 150 bases (one node counted
    more than 65 535 times); an assembly whose segments start at all 16 phases of a word.  -> dict: reads (codes, offs), counts, seqs, at
    (name -> index of the sequence in seqs), want (records at min_count 2), cn, matrix (64 rows)"""
    K = NAMED_K
    tx, (rcodes, roffs) = _reads(synth, K, 40, 4000, 150, (600, 150), seed=77)
    codes, starts, w = tx
    counts, kmers_in_reads, nodes = oracle_counts(rcodes, roffs, K)
    order = np.argsort(-w)                                # by expression: the first ones are covered hundreds of times
    T = lambda i: codes[int(starts[order[i]]):int(starts[order[i] + 1])]
    rng = np.random.default_rng(78)
    seqs, at = [], {}

    def add(name, s):
        at[name] = len(seqs)
        seqs.append(np.asarray(s, dtype=np.uint8))

    for i in range(8):
        add(f"whole{i}", T(i))
    add("revcomp1", revcomp(T(1)))                        # cn 2
    for c in range(2):
        add(f"copy2_{c}", T(2))                           # 3 copies with whole2
    for c in range(7):
        add(f"copy3_{c}", T(3))                           # 8 copies with whole3: column 7
    for total, i in ((4, 4), (5, 5), (6, 6)):             # columns 4, 5 and 6: a stretch of a transcript, `total` copies with the whole one
        for c in range(total - 1):
            add(f"stretch{total}_{c}", T(i)[100:300])
    mid = T(0)[200:560]                                   # well inside the most expressed transcript: solid all along
    add("straddle", substituted(mid, 79))                 # gap [49, 79]: across positions 63 | 64
    add("ends_at_63", substituted(mid, 63))               # gap [33, 63]
    add("starts_at_64", substituted(mid, 64 + K - 1))     # gap [64, 94]
    add("chimera", np.concatenate([T(0)[300:500], T(1)[300:500]]))
    add("random", rng.integers(0, 4, size=K + 199, dtype=np.uint8))        # one gap of 200 over four steps
    for L in (K - 1, K, K + 1, K + 62, K + 63, K + 64):
        add(f"len{L}", T(0)[600:600 + L])
    add("polyA", np.zeros(K + 299, dtype=np.uint8))       # 300 occurrences of one node: its byte is driven to 255
    long = np.concatenate([T(i) for i in range(8, 20)])
    assert len(long) >= 20000
    add("long", long[:20000])                             # more than 16 384 k-mers
    # every phase of a word: short fillers where the stream has not yet started a sequence at that phase
    phases = set()
    base = 0
    for s in seqs:
        phases.add(base % 16)
        base += len(s)
    for p in range(16):
        if p not in phases:
            pad = (p - base) % 16 or 16
            add(f"fill{p}a", T(7)[:pad + 16 * 3])         # moves the stream to phase p ...
            base += pad + 16 * 3
            add(f"fill{p}", T(7)[40:40 + K + 5])          # ... where this one starts
            base += K + 5
    want, cn = support(seqs, K, counts, NAMED_MIN_COUNT)
    return {"K": K, "reads": (rcodes, roffs), "counts": counts, "kmers_in_reads": kmers_in_reads, "nodes": nodes, "seqs": seqs, "at": at,
            "want": want, "cn": cn, "matrix": spectrum(counts, cn, NAMED_ROWS)}


@functools.lru_cache(maxsize=None)
def reduced_case(synth, K):
    """a small case per K: reads of 8 short transcripts (and 300 poly-A reads, so that one count passes 65 535 where the reads are long
    enough); whole transcripts, a reverse complement, a substitution, a chimera, random bases, lengths around K and around a step"""
    L = K + 110
    hot = (300, K + 250)                                  # 300 x 251 = 75 300 occurrences
    tx, (rcodes, roffs) = _reads(synth, K, 8, 1500, L, hot, seed=100 + K, lo=300, hi=700)
    codes, starts, w = tx
    counts, kmers_in_reads, nodes = oracle_counts(rcodes, roffs, K)
    order = np.argsort(-w)
    T = lambda i: codes[int(starts[order[i]]):int(starts[order[i] + 1])]
    rng = np.random.default_rng(K)
    seqs = [T(i) for i in range(5)] + [revcomp(T(1)), T(2), T(2), substituted(T(0)[:300], K + 48), np.concatenate([T(0)[20:150], T(1)[20:150]]),
                                       rng.integers(0, 4, size=K + 130, dtype=np.uint8), np.zeros(K + 280, dtype=np.uint8)]
    seqs += [T(0)[50:50 + n] for n in (0, 1, K - 1, K, K + 1, K + 62, K + 63, K + 64)]
    return {"K": K, "reads": (rcodes, roffs), "counts": counts, "kmers_in_reads": kmers_in_reads, "nodes": nodes,
            "seqs": [np.asarray(s, dtype=np.uint8) for s in seqs]}


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def parse_fasta(texts):
    """FASTA texts -> (segments, ref_of_seq, seg_start, names, bases): every letter outside ACGT cuts a contig; seg_start counts every
    letter of the record"""
    segs, ref_of_seq, seg_start, names, bases = [], [], [], [], []
    for text in texts:
        for record in text.split(">")[1:]:
            head, _, body = record.partition("\n")
            names.append(head.split()[0])
            letters = "".join(body.split())
            bases.append(sum(c in "ACGTacgt" for c in letters))
            cur, start = [], 0
            for i, c in enumerate(letters + "N"):
                if c in "ACGTacgt":
                    if not cur:
                        start = i
                    cur.append(c)
                elif cur:
                    segs.append(codes_of("".join(cur)))
                    ref_of_seq.append(len(names) - 1)
                    seg_start.append(start)
                    cur = []
    return segs, ref_of_seq, seg_start, names, bases


def support_text(rec, ref_of_seq, seg_start, names, bases):
    lines = []
    for i, (name, b) in enumerate(zip(names, bases)):
        mine = [j for j, r in enumerate(ref_of_seq) if r == i]
        f = {k: sum(int(rec[k][j]) for j in mine) for k in ("sum", "kmers", "found", "solid", "gaps")}
        best, best_at = 0, f["kmers"]
        for j in mine:
            if int(rec["longest_gap"][j]) > best:
                best, best_at = int(rec["longest_gap"][j]), seg_start[j] + int(rec["longest_at"][j])
        lines.append(f"{i + 1} {name} {b} {f['kmers']} {f['found']} {f['solid']} {f['sum']} {f['gaps']} {best} {best_at}\n")
    return "".join(lines)


def spectrum_text(matrix):
    return "".join(f"{r} " + " ".join(str(int(x)) for x in row) + "\n" for r, row in enumerate(matrix) if row.any())


def summary_fields(tot, matrix, min_count, K):
    """(S, N, F, V, D, E, C, P, Q): P and Q as text; Q is the Python value of the formula, or inf / -"""
    S, N, F, V = (int(x) for x in tot)
    D = int(matrix.sum())
    E = int(matrix[min_count:].sum())
    C = int(matrix[min_count:, 1:].sum())
    P = "-" if E == 0 else str(10000 * C // E)
    Q = "-" if N == 0 else ("inf" if V == N else str(int(math.floor(100 * -10 * math.log10(1 - (V / N) ** (1 / K)) + 0.5))))
    return S, N, F, V, D, E, C, P, Q
