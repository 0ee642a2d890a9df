"""GPU (-m gpu): `sdt-kmers support` on the built case of the bubble tests, written as FASTA, against the Python restatement of the rule
and of its outputs (unitig_support_util.py): prefix.unitigSupport, prefix.linkSupport, prefix.junctions and the summary line, byte for byte (the
tool adds single reads and writes no mate links); and the unitig files against what `sdt-kmers unitigs` writes from the same input."""
import pytest

import bubble_util as bu
import unitig_support_util as su
from test_unitig_thread_cli import library, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [31, 65])
def test_sdt_kmers_support_cli(pkg, tmp_path, K):
    case = bu.built_case(K)
    cfg = library(tmp_path, case)
    for name, args, (mc, ml) in (("a", [], (2, 1)), ("b", ["-c", "1", "--max-junctions", "64"], (1, 1))):
        sup = su.bubble_support(K, mc, ml)
        lines = run(pkg, "support", cfg, K, tmp_path / name, *args)
        run(pkg, "unitigs", cfg, K, tmp_path / (name + "_u"), *args[:2])
        assert (tmp_path / f"{name}.unitigSupport").read_text() == su.unitig_support_text(sup), f"K={K} {name}.unitigSupport"
        assert (tmp_path / f"{name}.linkSupport").read_text() == su.link_support_text(sup), f"K={K} {name}.linkSupport"
        assert (tmp_path / f"{name}.junctions").read_text() == su.junctions_text(sup) != "", f"K={K} {name}.junctions"
        assert not (tmp_path / f"{name}.mateLinks").exists()
        assert [x for x in lines if x.startswith("support: ")] == [su.summary_line(sup)]
        for ext in ("unitigs", "unitigs.fa", "unitigs.gfa"):
            assert (tmp_path / f"{name}.{ext}").read_bytes() == (tmp_path / f"{name}_u.{ext}").read_bytes(), ext
