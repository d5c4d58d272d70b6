"""Output-format parity with the reference and the getAvgs.sh re-implementation,
checked against the reference's own recorded results (tests/golden/reference_mpi: its raw outputs,
collected.txt and results/, text files)."""
import os

import pytest

from cuda_mpi_reductions_amd.utils import formats, getavgs

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_mpi")


def test_gnuplot_line_matches_reduce_c_printf():
    # reduce.c:81 printf("INT %s %d %10.3lf\n", ...)
    assert formats.gnuplot_line("INT", "SUM", 1024, 146.684) == "INT SUM 1024    146.684"
    assert formats.gnuplot_line("DOUBLE", "MAX", 64, 5.6) == "DOUBLE MAX 64      5.600"
    assert formats.GNUPLOT_HEADER == "# DATATYPE OP NODES GB/sec"


def test_throughput_line_matches_reduction_cpp():
    line = formats.throughput_line(92.7729, 0.00072, 16777216, 1, 256)
    assert line == ("Reduction, Throughput = 92.7729 GB/s, Time = 0.00072 s, Size = 16777216 Elements, "
                    "NumDevsUsed = 1, Workgroup = 256")
    assert formats.parse_throughput(line)["elements"] == 16777216


def test_parse_reference_raw_outputs():
    rows = []
    for name in sorted(os.listdir(os.path.join(REF, "raw_output"))):
        with open(os.path.join(REF, "raw_output", name)) as f:
            rows += list(formats.parse_gnuplot(f))
    assert len(rows) > 300
    assert {r.dtype for r in rows} == {"INT", "DOUBLE"}
    assert {r.op for r in rows} == {"MAX", "MIN", "SUM"}


def test_getavgs_reproduces_reference_results(tmp_path):
    getavgs.write_results(os.path.join(REF, "collected.txt"), str(tmp_path))
    for dt in ("INT", "DOUBLE"):
        for op in ("SUM", "MIN", "MAX"):
            ours = open(tmp_path / f"{dt}_{op}.txt").read().splitlines()
            theirs = open(os.path.join(REF, "results", f"{dt}_{op}.txt")).read().splitlines()
            assert ours[0] == theirs[0] == ""
            # Same lines; the shipped files list rank counts in descending order although the
            # script's `sort -n` sorts ascending — compare as sets and document (docs/PARITY.md).
            assert sorted(ours[1:]) == sorted(theirs[1:])


def test_bc_division_truncates_like_bc():
    assert getavgs.bc_div("1", 3) == ".33333"
    assert getavgs.bc_div("10", 3) == "3.33333"
    assert getavgs.bc_div("-2", 3) == "-.66666"


def test_python_cli_grammar():
    from cuda_mpi_reductions_amd.utils import cli
    a = cli.parse(["--method=SUM", "-type=double", "--cpufinal", "-n=1M"])
    assert cli.get_str(a, "method") == "SUM" and cli.get_str(a, "type") == "double"
    assert cli.has(a, "cpufinal") and cli.get_str(a, "cpufinal") is None
    assert cli.get_int(a, "n") == 1 << 20
    assert cli.parse_count("1e9") == 10**9 and cli.parse_count("4k") == 4096
    with pytest.raises(cli.CliError):
        cli.parse(["method=SUM"])


def test_getavgs_averages_the_co_mode_raw_outputs():
    """The BG/L CO-mode runs were never averaged by the reference's authors:
    getAvgs over the concatenated `stdout-co-*` files gives the table the survey quotes."""
    lines = []
    for name in sorted(os.listdir(os.path.join(REF, "raw_output"))):
        if name.startswith("stdout-co-"):
            with open(os.path.join(REF, "raw_output", name)) as f:
                lines += f.readlines()
    avgs = getavgs.averages(lines)
    expect = {  # SURVEY.md §6.3, GiB/s, 3 decimals
        ("INT", "SUM"): {32: 10.037, 128: 40.142, 512: 160.437},
        ("INT", "MIN"): {32: 9.743, 128: 38.967, 512: 155.720},
        ("INT", "MAX"): {32: 9.743, 128: 38.965, 512: 155.675},
        ("DOUBLE", "SUM"): {32: 5.396, 128: 21.515, 512: 84.944},
        ("DOUBLE", "MIN"): {32: 2.977, 128: 11.909, 512: 48.937},
        ("DOUBLE", "MAX"): {32: 2.978, 128: 11.937, 512: 48.685},
    }
    for key, by_nodes in expect.items():
        got = {n: float(v) for n, v in avgs[key]}
        assert set(got) == set(by_nodes), (key, got)
        for n, v in by_nodes.items():
            assert abs(got[n] - v) <= 1.5e-3, (key, n, got[n], v)  # survey: rounded; bc: truncated
