"""The reference screen (include/sdt_gpu.h, "Reads screened against reference sequences") restated in plain Python: a dict from canonical
k-mer to the smallest reference that holds it, and the rule of a read and of a unit.  Integers only; nothing here comes from the
library.  Bases are the stream's codes."""
import functools

import numpy as np

A, C, T, G = 0, 1, 2, 3
NO_REF = 0xFFFFFFFF
KEEP_MATCHED = 1
KEPT, DROPPED = 0, 1
KS = (11, 16, 21, 31)
N_REFS = 6
FIELDS = ("kmers", "hits", "ref", "start", "len", "verdict")
DTYPE = np.dtype([(f, np.uint32) for f in FIELDS])


def params(min_hits=1, min_hit_pct=0, flags=0, reserved=0):
    return dict(min_hits=min_hits, min_hit_pct=min_hit_pct, flags=flags, reserved=reserved)


def revcomp(codes):
    return (np.asarray(codes, dtype=np.uint8)[::-1] ^ 2).astype(np.uint8)


def kmer_int(codes):
    v = 0
    for c in codes:
        v = v << 2 | int(c)
    return v


def revcomp_int(x, k):
    r = 0
    for _ in range(k):
        r = r << 2 | ((x & 3) ^ 2)
        x >>= 2
    return r


def canonical_kmers(codes, k):
    """the canonical k-mer at every position of codes: a list of max(len - k + 1, 0) integers"""
    out = []
    fw = rc = 0
    mask = (1 << 2 * k) - 1
    top = 2 * (k - 1)
    for i, c in enumerate(codes):
        c = int(c)
        fw = (fw << 2 | c) & mask
        rc = rc >> 2 | (c ^ 2) << top
        if i >= k - 1:
            out.append(fw if fw < rc else rc)
    return out


def build_set(seqs, refs, k):
    """canonical k-mer -> the smallest reference among the sequences that hold it or its reverse complement"""
    d = {}
    for s, r in zip(seqs, refs):
        for x in canonical_kmers(s, k):
            if d.get(x, NO_REF) > r:
                d[x] = int(r)
    return d


def positions(seqs, k):
    return sum(max(len(s) - k + 1, 0) for s in seqs)


def concat(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        offs[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    codes = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]) if reads else np.zeros(0, dtype=np.uint8)
    return codes.astype(np.uint8), offs


def read_facts(codes, k, d):
    """(kmers, hits, ref) of one read"""
    km = canonical_kmers(codes, k)
    found = [d[x] for x in km if x in d]
    return len(km), len(found), min(found) if found else NO_REF


def read_matched(kmers, hits, p):
    return hits >= max(p["min_hits"], 1) and 100 * hits >= p["min_hit_pct"] * kmers


def verdicts(facts, lens, p, units):
    """facts: (kmers, hits, ref) per read, units: lists of read indices -> (records, keep, kept)"""
    rec = np.zeros(len(facts), dtype=DTYPE)
    keep = np.zeros(len(facts), dtype=np.uint8)
    for u in units:
        m = any(read_matched(facts[i][0], facts[i][1], p) for i in u)
        dropped = (not m) if p["flags"] & KEEP_MATCHED else m
        for i in u:
            rec[i] = (facts[i][0], facts[i][1], facts[i][2], 0, 0 if dropped else lens[i], DROPPED if dropped else KEPT)
            keep[i] = 0 if dropped else 1
    return rec, keep, int(keep.sum())


def dense_units(n, paired):
    return [[2 * t, 2 * t + 1] for t in range(n // 2)] if paired else [[i] for i in range(n)]


def expect_screen(codes, offs, k, d, p, paired=False, facts=None):
    """the dense forms -> (records, keep, kept); facts: what all_facts gave for these reads (they do not depend on p)"""
    n = len(offs) - 1
    facts = facts if facts is not None else all_facts(codes, offs, k, d)
    lens = [int(offs[i + 1]) - int(offs[i]) for i in range(n)]
    return verdicts(facts, lens, p, dense_units(n, paired))


def all_facts(codes, offs, k, d):
    return [read_facts(codes[int(offs[i]):int(offs[i + 1])], k, d) for i in range(len(offs) - 1)]


def ranged_units(present, pair_ranges):
    """the kept form: present: the ordinals that have a read (any order); a pair of a range with one mate present is a unit of that read"""
    have = set(int(o) for o in present)
    paired_with = {}
    for first, end in pair_ranges:
        for o in range(int(first), int(end), 2):
            if o in have and o + 1 in have:
                paired_with[o] = o + 1
    units, done = [], set()
    for o in sorted(have):
        if o in done:
            continue
        if o in paired_with:
            units.append([o, paired_with[o]])
            done.add(paired_with[o])
        else:
            units.append([o])
    return units


def assert_records_equal(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} records, {len(want)} expected"
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{what}: {f} differs at {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()}, want {want[f][bad[:8]].tolist()}"


def cut_kept(codes, offs, rec):
    return [codes[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1) if rec["verdict"][i] == KEPT]


# ---- the named set: about 40 sequences over 6 references -------------------------------------------------------------------------
SET_POSITIONS = 31500                                    # k-mer positions of the set at every k: 96 % of 32 768 slots when forced


@functools.lru_cache(maxsize=None)
def set_case(k):
    """-> dict(seqs, refs, shared, pal): one sequence of 20 000 bases and one of 6 000; sequences of k - 1, k, k + 1, 3 and 0 bases; two
    segments of reference 3; the k-mer `shared` in references 4 and 1 and its reverse complement in 2; the all-A k-mer in reference 5
    and the all-T one in 3; a palindrome of 16 bases; 16 sequences of 49 bases, so that a sequence starts at every base of a word;
    one last sequence that brings the k-mer positions to SET_POSITIONS"""
    rng = np.random.default_rng(1000 + k)
    seq = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    shared = seq(k)
    half = seq(8)
    pal = np.concatenate([half, revcomp(half)])
    items = [(seq(20000), 0), (seq(6000), 1), (seq(k - 1), 2), (seq(k), 2), (seq(k + 1), 3), (seq(3), 0), (seq(0), 5),
             (seq(300), 3), (seq(170), 3),
             (np.concatenate([seq(40), shared, seq(33)]), 4), (np.concatenate([seq(21), shared, seq(50)]), 1),
             (np.concatenate([seq(35), revcomp(shared), seq(18)]), 2),
             (np.concatenate([seq(30), np.full(k, A, dtype=np.uint8), seq(30)]), 5), (np.concatenate([seq(25), np.full(k + 2, T, dtype=np.uint8), seq(9)]), 3),
             (np.concatenate([seq(19), pal, seq(27)]), 4)]
    items += [(seq(int(rng.integers(40, 400))), int(rng.integers(0, N_REFS))) for _ in range(9)]
    items += [(seq(49), i % N_REFS) for i in range(16)]
    seqs, refs = [s for s, _ in items], [r for _, r in items]
    short = SET_POSITIONS - positions(seqs, k)
    assert short > 100
    seqs.append(seq(short + k - 1))
    refs.append(0)
    assert positions(seqs, k) == SET_POSITIONS and len(seqs) == 41
    return dict(seqs=seqs, refs=refs, shared=shared, pal=pal)


@functools.lru_cache(maxsize=None)
def set_dict(k):
    c = set_case(k)
    return build_set(c["seqs"], c["refs"], k)


def absent_kmers(k, d, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x = int(rng.integers(0, 1 << 62)) & ((1 << 2 * k) - 1)
        if min(x, revcomp_int(x, k)) not in d:
            out.append(x)
    return out


# ---- the named reads: every length at which the kernel takes another path, of three kinds, and their reverse complements ------------
@functools.lru_cache(maxsize=None)
def read_case(k, seed=None):
    """-> dict(reads, codes, offs, facts, exact): reads of 0, k - 1, k, k + 1, k + 63, k + 64, 200 and 5 000 bases, cut from the references,
    random, and half of each; then the reverse complement of every one; then a read of k + 99 bases (100 k-mers) whose first k + 36
    bases are a reference's.  exact: its index.  seed: another draw of the same generator"""
    rng = np.random.default_rng(2000 + k if seed is None else seed)
    c = set_case(k)
    big = c["seqs"][0]
    reads = []
    for L in (0, k - 1, k, k + 1, k + 63, k + 64, 200, 5000):
        at = int(rng.integers(0, len(big) - L + 1))
        cut = big[at:at + L].copy()
        rnd = rng.integers(0, 4, size=L, dtype=np.uint8)
        half = np.concatenate([cut[:L // 2], rnd[L // 2:]])
        reads += [cut, rnd, half]
    # reads that meet other references: the shared k-mer, poly-A, the palindrome
    reads += [np.concatenate([rng.integers(0, 4, size=20, dtype=np.uint8), c["shared"], rng.integers(0, 4, size=20, dtype=np.uint8)]),
              np.full(k + 5, A, dtype=np.uint8), np.full(k + 5, T, dtype=np.uint8), c["seqs"][1][100:100 + 150].copy()]
    reads += [revcomp(r) for r in reads]
    at = int(rng.integers(0, len(big) - (k + 36)))
    reads.append(np.concatenate([big[at:at + k + 36], rng.integers(0, 4, size=63, dtype=np.uint8)]))
    codes, offs = concat(reads)
    facts = all_facts(codes, offs, k, set_dict(k))
    return dict(reads=reads, codes=codes, offs=offs, facts=facts, exact=len(reads) - 1)


# ---- the host program: the reference files and the four texts ---------------------------------------------------------------------
LETTERS = "ACTG"


def parse_refs(texts):
    """FASTA texts in the order of the command line -> (segments, ref_of_seq, names, bases): a letter other than ACGT (either case)
    cuts a reference; the name is the header up to the first blank; bases counts the letters ACGT"""
    code = {"A": A, "C": C, "T": T, "G": G}
    seqs, refs, names, bases = [], [], [], []
    for text in texts:
        body = None
        records = []
        for line in text.split("\n"):
            if line.startswith(">"):
                body = []
                records.append((line[1:].split()[0] if line[1:].split() else "", body))
            elif line.strip():
                assert body is not None, "bases before the first header"
                body.append("".join(line.split()))
        for name, body in records:
            letters = "".join(body).upper()
            assert letters, "a record without sequence"
            names.append(name)
            bases.append(sum(letters.count(x) for x in "ACGT"))
            seg = []
            for ch in letters + "N":
                if ch in code:
                    seg.append(code[ch])
                elif seg:
                    seqs.append(np.array(seg, dtype=np.uint8))
                    refs.append(len(names) - 1)
                    seg = []
    return seqs, refs, names, bases


def cli_texts(codes, offs, rec, pair_ranges, names, bases, p):
    """the four files of `sdt-kmers screen` for a stream in ordinal order: (readScreen, pairs.fa, single.fa, screenStats)"""
    n = len(offs) - 1
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)[codes].tobytes().decode()
    one = lambda r: 0 if r == NO_REF else int(r) + 1
    rec_txt = "".join(f"{c['kmers']} {c['hits']} {one(c['ref'])} {c['verdict']}\n" for c in rec)
    mate = {}
    for first, end in pair_ranges:
        for r in range(first, end, 2):
            mate[r], mate[r + 1] = r + 1, r
    pairs, single = [], []
    for r in range(n):
        if rec["verdict"][r] == KEPT and rec["len"][r]:
            both = r in mate and rec["verdict"][mate[r]] == KEPT and rec["len"][mate[r]] > 0
            (pairs if both else single).append(f">{r + 1}\n{letters[int(offs[r]):int(offs[r + 1])]}\n")
    stats = ""
    for i, (name, b) in enumerate(zip(names, bases)):
        mine = (rec["ref"] == i) & (rec["hits"] > 0)
        stats += f"{i + 1} {name} {b} {int(mine.sum())} {int(rec['hits'][mine].sum())}\n"
    matched = sum(read_matched(int(c["kmers"]), int(c["hits"]), p) for c in rec)
    v = rec["verdict"]
    stats += f"# reads {n} matched {matched} kept {int((v == KEPT).sum())} dropped {int((v == DROPPED).sum())}\n"
    return rec_txt, "".join(pairs), "".join(single), stats
