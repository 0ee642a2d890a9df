"""GPU (-m gpu): `sdt-kmers cluster` on a library of single reads and a library of a pair of files, against the Python restatement of
the rule and of the four files (read_cluster_util.py): the files and the summary line, --pick, and two runs byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import read_cluster_util as cu

pytestmark = pytest.mark.gpu

K, L = 31, 100


def write_fastq(path, reads, tag):
    letters = np.frombuffer(cu.LETTERS.encode(), dtype=np.uint8)
    with open(path, "wb") as fo:
        for i, r in enumerate(reads):
            fo.write(b"@r%d%s\n%s\n+\n%s\n" % (i, tag.encode(), letters[r].tobytes(), b"I" * len(r)))


def library(tmp_path):
    """an odd number of single reads (q=, the smaller avg_ins: streamed first, so the pairs start at an odd ordinal): six transcripts
    tiled on both strands, one of them with a chimeric read into the next, random reads and reads shorter than K; and pairs (q1= / q2=)
    of mates from one transcript, from two, with a random mate and with a short one.  Returns the config, the stream in ordinal order
    and the pair ranges"""
    rng = np.random.default_rng(131)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    tx = [rnd(int(rng.integers(300, 601))) for _ in range(6)]
    singles = []
    for t in tx:
        singles += cu.tiled(t, L, step=20)
    singles += [np.concatenate([tx[0][-50:], tx[1][:50]]), rnd(L), rnd(70), rnd(25), tx[2][:K - 1], tx[3][40:40 + K]]
    if len(singles) % 2 == 0:
        singles.append(rnd(60))
    r1, r2 = [], []
    for i in range(24):
        t = tx[i % 6]
        r1.append(t[:L])
        r2.append(cu.revcomp(t[len(t) - L:]))
    r1 += [tx[0][:L], rnd(L), tx[4][:L], rnd(20), rnd(L), tx[5][:80]]
    r2 += [tx[3][:L], tx[2][:L], rnd(L), tx[1][:L], rnd(L), rnd(20)]
    write_fastq(tmp_path / "s.fq", singles, "")
    write_fastq(tmp_path / "p_1.fq", r1, "/1")
    write_fastq(tmp_path / "p_2.fq", r2, "/2")
    cfg = tmp_path / "lib.cfg"
    cfg.write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 's.fq'}\n"
                   f"[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nq1={tmp_path / 'p_1.fq'}\nq2={tmp_path / 'p_2.fq'}\n")
    stream = singles + [r for pair in zip(r1, r2) for r in pair]
    return str(cfg), stream, [(len(singles), len(singles) + 2 * len(r1))]


def run(pkg, cfg, out, *more):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "cluster", "-s", cfg, "-K", str(K), "-p", "4", "-o", str(out)] + list(more), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


EXTS = ("readCluster", "clusters", "cluster.pairs.fa", "cluster.single.fa")


def test_sdt_kmers_cluster_cli(pkg, tmp_path):
    cfg, stream, ranges = library(tmp_path)
    n = len(stream)
    first, end = ranges[0]
    assert first & 1
    codes, offs = cu.concat(stream)
    nodes = cu.oracle_nodes(cu.counted_oracle(codes, offs, K))
    units = [[i] for i in range(first)] + [[i, i + 1] for i in range(first, end, 2)]
    lengths = [len(r) for r in stream]
    for name, args, prm in (("a", [], dict(min_count=2, max_count=0, min_link=1)), ("b", ["-c", "3", "--max-count", "8", "--min-link", "2"], dict(min_count=3, max_count=8, min_link=2))):
        model = cu.Clustering(nodes, K, **prm)
        rec = model.records(stream, units=units)[0]
        assert set(rec["verdict"].tolist()) == {0, 1, 2, 3, 4} and model.info[2] >= 6 and (name == "a") == (model.info[2] == 6)
        lines = run(pkg, cfg, tmp_path / name, *args)
        pairs_txt, single_txt = cu.fasta_texts(stream, rec, np.ones(n, dtype=bool), ranges)
        want = (cu.read_cluster_text(rec), cu.clusters_text(model, rec, lengths), pairs_txt, single_txt)
        for ext, text in zip(EXTS, want):
            got = (tmp_path / f"{name}.{ext}").read_text()
            assert got == text, f"{name}.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
        assert [x for x in lines if x.startswith("cluster: ")] == [cu.summary_line(model, rec)]
        assert pairs_txt.count(">") == end - first and single_txt.count(">") == first
    assert (tmp_path / "a.clusters").read_text() != (tmp_path / "b.clusters").read_text()
    # --pick: the units of clusters 2 .. 4 alone; the record lines and the cluster list are those of the whole stream
    model = cu.Clustering(nodes, K, 2, 0, 1)
    rec, keep, kept = model.records(stream, units=units, pick=(1, 3))
    assert 0 < kept < n and keep[first:end].any() and keep[:first].any()
    run(pkg, cfg, tmp_path / "p", "--pick", "2:4")
    pairs_txt, single_txt = cu.fasta_texts(stream, rec, keep, ranges)
    for ext, text in zip(EXTS, (cu.read_cluster_text(rec), cu.clusters_text(model, rec, lengths), pairs_txt, single_txt)):
        assert (tmp_path / f"p.{ext}").read_text() == text, ext
    assert pairs_txt.count(">") + single_txt.count(">") == kept
    # a second run writes the same bytes
    run(pkg, cfg, tmp_path / "again")
    for ext in EXTS:
        assert (tmp_path / f"again.{ext}").read_bytes() == (tmp_path / f"a.{ext}").read_bytes(), ext
