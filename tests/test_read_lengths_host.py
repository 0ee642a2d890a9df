"""CPU: the checkers at long reads.  The oracle's pass-1 driver (sdto_sets_add_read) used to cut every read to 8 192 bases without a
word; the GPU tests of tests/test_read_lengths.py lean on it for reads of up to 16 384 + K bases, so its own ceiling goes first: a
20 000-base read against a plain dict of canonical k-mers that shares nothing with the oracle but the base coding."""
import numpy as np
import pytest

import oracle_binding as ob


def canonical_counts(codes, K):
    """{canonical k-mer as an int (2 bits per base, first base most significant): occurrences} of one read; complement = code ^ 2"""
    mask = (1 << (2 * K)) - 1
    fw = rv = 0
    out = {}
    for i, b in enumerate(int(x) for x in codes):
        fw = ((fw << 2) | b) & mask
        rv = (rv >> 2) | ((b ^ 2) << (2 * (K - 1)))
        if i >= K - 1:
            k = min(fw, rv)
            out[k] = out.get(k, 0) + 1
    return out


def keys_to_int(keys):
    out = []
    for row in keys:
        v = 0
        for x in row:
            v = (v << 64) | int(x)
        out.append(v)
    return out


@pytest.mark.parametrize("K", [31, 95])
def test_oracle_counts_a_20000_base_read_whole(K):
    L = 20_000
    rng = np.random.default_rng(K)
    unit = rng.integers(0, 4, size=7_000, dtype=np.uint8)
    # a repeat past the old 8 192-base cut (counts > 1 that only the read's far end produces), then random bases to the end
    codes = np.concatenate([unit, rng.integers(0, 4, size=3_000, dtype=np.uint8), unit[1000:5000],
                            rng.integers(0, 4, size=L - 14_000, dtype=np.uint8)])
    assert len(codes) == L
    want = canonical_counts(codes, K)
    assert sum(want.values()) == L - K + 1 and max(want.values()) >= 2
    o = ob.Oracle(K, nsets=3)
    # a short read first and last: the buffers grow in the middle of a stream, and a read after the long one is whole too
    short = rng.integers(0, 4, size=K + 5, dtype=np.uint8)
    for k, v in canonical_counts(short, K).items():
        want[k] = want.get(k, 0) + 2 * v
    allc = np.concatenate([short, codes, short])
    offs = np.array([0, K + 5, K + 5 + L, 2 * (K + 5) + L], dtype=np.uint64)
    o.add_reads(allc, offs)
    assert o.kmers_in_reads() == L - K + 1 + 2 * 6
    assert o.node_count() == len(want)
    keys, _, _, cnt, _ = o.export()
    assert dict(zip(keys_to_int(keys), (int(c) for c in cnt))) == want
    # first-occurrence ordinals of the long read (read 1): positions past 8 192 are there, none past the read's last k-mer
    first = o.export_first()
    pos1 = sorted(int(f) & 0xFFFF for f in first if int(f) >> 16 == 1)
    assert pos1[-1] == L - K and len(pos1) > 15_000
