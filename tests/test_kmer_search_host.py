"""CPU: the k-mer search / read profile entry points exist at every layer (header, library, binding, host program), and
sdt-kmers checks its query file before it touches a device -- so all of this runs on a box without a GPU."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_search_kmers", "sdt_gpu_search_kmers_device", "sdt_gpu_profile_reads", "sdt_gpu_profile_reads_device",
           "sdt_gpu_profile_kept_reads"]


def test_header_declares_and_library_exports_the_five_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+kmers,\s*found,\s*solid,\s*min,\s*median,\s*max;\s*\}\s*sdt_read_cov;", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_read_cov_dtype_is_the_c_struct(pkg):
    dt = pkg.READ_COV_DTYPE
    assert dt.itemsize == 24
    assert dt.names == ("kmers", "found", "solid", "min", "median", "max")
    assert all(dt.fields[n][0] == np.uint32 and dt.fields[n][1] == 4 * i for i, n in enumerate(dt.names))
    for m in ("search_kmers", "profile_reads", "profile_kept_reads"):
        assert callable(getattr(pkg.PregraphGPU, m))


def sdt_kmers(pkg):
    subprocess.run(["make", "-C", pkg.CSRC_DIR], check=True, stdout=subprocess.DEVNULL)
    p = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    assert os.path.exists(p), "make -C csrc does not build sdt-kmers"
    return p


def test_make_builds_sdt_kmers_and_it_prints_usage(pkg):
    exe = sdt_kmers(pkg)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "usage" in r.stderr and "profile" in r.stderr and "query" in r.stderr
    r = subprocess.run([exe, "frobnicate", "-s", "x"], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr
    r = subprocess.run([exe, "profile", "-s", "x.cfg", "-K", "31"], capture_output=True, text=True)      # no -o
    assert r.returncode != 0 and "usage" in r.stderr


def test_query_file_is_checked_before_the_device_is_touched(pkg, tmp_path):
    """a k-mer of the wrong length, or with an N in it: exit status 2 and the line is named -- with no device present (the
    config does not even exist: the query file comes first)"""
    exe = sdt_kmers(pkg)
    good = "ACGTTGCATGCATGCATTGCA"                       # 21 letters
    q = tmp_path / "q.txt"
    q.write_text(good + "\n" + good.lower() + "\n\n" + good[:-1] + "\n")
    r = subprocess.run([exe, "query", "-s", str(tmp_path / "none.cfg"), "-K", "21", "-q", str(q)], capture_output=True, text=True)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "line 4" in r.stderr and "20 letters" in r.stderr
    q.write_text(good + "\n" + good[:7] + "N" + good[8:] + "\n")
    r = subprocess.run([exe, "query", "-s", str(tmp_path / "none.cfg"), "-K", "21", "-q", str(q)], capture_output=True, text=True)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "line 2" in r.stderr and "'N'" in r.stderr
    # K is clamped as pregraph.c:38-59 does before the letters are counted: -K 20 means 21
    q.write_text(good + "\n")
    r = subprocess.run([exe, "query", "-s", str(tmp_path / "none.cfg"), "-K", "20", "-q", str(q)], capture_output=True, text=True)
    assert r.returncode not in (0, 2), (r.returncode, r.stderr)      # the file is fine: it is the config that is missing
    r = subprocess.run([exe, "query", "-s", str(tmp_path / "none.cfg"), "-K", "21", "-q", str(tmp_path / "absent.txt")], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot open" in r.stderr
