"""CPU: the device-free half of `sdt-kmers` that every read stage shares -- the walk over the kept reads by ordinal (csrc/host/readwalk.c)
as a stand-alone program under sanitizers, and which subcommand may be given which option, against the built tool."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUBCOMMANDS = ("profile", "query", "correct", "normalize", "trim", "dedup", "clip", "overlap", "complexity", "qtrim", "screen")
# (options with a valid value, the subcommands that take them, the text after "belongs to")
OWNERSHIP = (
    ((("--target", "5"), ("--max-cv", "100"), ("--seed", "1")), ("normalize",), "normalize"),
    ((("--min-cov", "3"), ("--correct",)), ("trim",), "trim"),
    ((("--min-len", "50"),), ("trim", "clip", "overlap", "complexity", "qtrim"), "trim, clip, overlap, complexity and qtrim"),
    ((("-a", "{fa}"), ("-g", "{fa}"), ("--tail3", "A"), ("--tail5", "T"), ("--error-pct", "10"), ("--min-tail", "10"), ("--tail-error-pct", "20")),
     ("clip",), "clip"),
    ((("--min-overlap", "5"),), ("clip", "overlap"), "clip"),
    ((("--max-err", "10"),), ("overlap",), "overlap"),
    ((("--max-score", "5"), ("--max-low", "30"), ("--trim-low",)), ("complexity",), "complexity"),
    ((("--phred", "33"), ("--cut-q", "20"), ("--low-q", "15"), ("--max-low-bases", "40"), ("--max-ee", "1000")), ("qtrim",), "qtrim"),
    ((("-r", "{fa}"), ("--screen-k", "21"), ("--min-hits", "2"), ("--min-hit-pct", "5"), ("--keep-matched",)), ("screen",), "screen"),
    ((("--mate-swap",),), ("dedup",), "dedup"),
)


def test_walk_over_the_kept_reads_clean_under_sanitizers(tmp_path):
    """tools/readwalk_host_check.c: hand-made kept batches through the one walk by ordinal (csrc/host/readwalk.c): the three texts, the
    refusals, a record across the block boundary and a write failure; a stand-alone program built with AddressSanitizer + UBSan and run
    on the CPU"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "readwalk_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "readwalk_host_check.c"), os.path.join(host, "readwalk.c"),
                    os.path.join(host, "trimsplit.c"), os.path.join(host, "normsplit.c")], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "readwalk_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_sdt_kmers_polices_every_option_of_every_subcommand(pkg, tmp_path):
    """the whole matrix: an option given to a subcommand that does not take it is refused by name with exit code 255, one given to a
    subcommand that takes it is not; either way before anything is written (the config path is never opened)"""
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    cfg, out, fa = str(tmp_path / "none.cfg"), str(tmp_path / "out"), str(tmp_path / "none.fa")
    seen = 0
    for sub in SUBCOMMANDS:
        for opts, owners, text in OWNERSHIP:
            for opt in opts:
                args = [a.format(fa=fa) for a in opt]
                r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", *args, "-o", out], capture_output=True, text=True)
                if sub in owners:
                    assert "belongs to" not in r.stderr, f"{sub} {args}: {r.returncode} {r.stderr[:200]}"
                    assert r.returncode != 0                     # (the adapter, reference, query or config file is not there)
                else:
                    assert r.returncode == 255 and f"sdt-kmers: {opt[0]} belongs to {text}\n" in r.stderr, f"{sub} {args}: {r.returncode} {r.stderr[:200]}"
                seen += 1
    assert seen == len(SUBCOMMANDS) * 29
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
