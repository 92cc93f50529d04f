"""tools/benchkit.py without a device: the A/B comparison on the recorded runs of the vertical-difference refactor
(profiles/vderiv_cell/, the table of profiles/README.md), what it refuses and what it flags, the order of work of the one
timing loop on a recording context, and the rounding of the statistics."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCHKIT = os.path.join(ROOT, "tools", "benchkit.py")
RUNS = os.path.join(ROOT, "profiles", "vderiv_cell")


@pytest.fixture(scope="module")
def bk():
    """The module; its preamble (the path, MIFC_LIB_PATH) is for the tools and is taken back for the rest of the suite."""
    path, lib = list(sys.path), os.environ.get("MIFC_LIB_PATH")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import benchkit
    finally:
        sys.path[:] = path
        if lib is None:
            os.environ.pop("MIFC_LIB_PATH", None)
        else:
            os.environ["MIFC_LIB_PATH"] = lib
    return benchkit


def compare(*paths):
    r = subprocess.run([sys.executable, BENCHKIT, "compare", *paths], capture_output=True, text=True)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines()], r.stderr


def recorded(tool, which, run):
    return os.path.join(RUNS, "bench_%s_%s_%d.txt" % (tool, which, run))


def rewritten(tmp_path, path, edit):
    """A copy of a recorded run whose JSON rows went through edit(rows)."""
    with open(path) as f:
        rows = [json.loads(line) for line in f]
    edit(rows)
    copy = tmp_path / "edited.txt"
    copy.write_text("".join(json.dumps(r) + "\n" for r in rows))
    return str(copy)


# tool: row pairs, slower, without spread, median, largest and smallest ratio of the medians (profiles/README.md)
TABLE = {"pvort": (36, 0, 0, 1.0004, 1.0066, 0.982), "vderiv": (144, 0, 0, 0.999, 1.0511, 0.9789), "vlayer": (60, 0, 0, 0.9998, 1.0851, 0.985),
         "vinterp": (16, 0, 16, 0.9997, 1.0049, 0.9763)}


@pytest.mark.parametrize("tool", sorted(TABLE))
def test_compare_reproduces_the_recorded_table(tool):
    status, lines, err = compare(*(recorded(tool, which, run) for run in (1, 2) for which in ("parent", "new")))
    assert status == 0, err
    rows, slower, unjudged, median, largest, smallest = TABLE[tool]
    assert lines[-1] == {"rows": rows, "slower_beyond_the_two_spreads": slower, "without_spread": unjudged, "median_ratio": median,
                         "largest_ratio": largest, "smallest_ratio": smallest}
    assert len(lines) == rows + 1
    verdicts = [line["not_slower_beyond_the_two_spreads"] for line in lines[:-1]]
    assert verdicts == ["no spread" if unjudged else True] * rows  # a row without a spread is not a pass


def test_compare_refuses_a_missing_row(tmp_path):
    parent = recorded("vderiv", "parent", 1)
    status, lines, err = compare(parent, rewritten(tmp_path, parent, lambda rows: rows.pop(5)))
    assert status not in (0, 1) and not lines
    assert "different numbers of rows: 132 in" in err and ", 131 in" in err  # 72 measurement rows and 60 comparison lines


def test_compare_refuses_another_case(tmp_path):
    parent = recorded("pvort", "parent", 1)

    def edit(rows):
        assert rows[4]["method"] == "weighted"
        rows[4]["method"] = "centred"

    status, lines, err = compare(parent, rewritten(tmp_path, parent, edit))
    assert status not in (0, 1)
    assert "row 5" in err and "method is 'weighted' and 'centred'" in err
    assert len(lines) == 4  # the rows before it were paired


def test_compare_refuses_other_keys(tmp_path):
    parent = recorded("pvort", "parent", 1)
    status, _, err = compare(parent, rewritten(tmp_path, parent, lambda rows: rows[-1].pop("form")))  # a comparison line: its keys count too
    assert status not in (0, 1) and "different keys" in err
    # the one key a new run may add: the spread bench_vinterp.py did not print
    vinterp = recorded("vinterp", "parent", 1)

    def edit(rows):
        for r in rows:
            if "algorithmic_bytes" in r:
                r["kernel_ms_spread"] = 0.01

    status, lines, err = compare(vinterp, rewritten(tmp_path, vinterp, edit))
    assert status == 0, err
    assert lines[-1]["rows"] == lines[-1]["without_spread"] == 8
    status, _, err = compare(rewritten(tmp_path, vinterp, edit), vinterp)  # but a new run may not lose it
    assert status not in (0, 1) and "different keys" in err


def test_compare_flags_a_slower_row(tmp_path):
    parent = recorded("vderiv", "parent", 1)

    def edit(rows):
        r = rows[7]
        r["kernel_ms_min"] = round(r["kernel_ms_min"] + 2 * r["kernel_ms_spread"] + 0.0002, 4)  # above the minimum plus the two spreads

    status, lines, err = compare(parent, rewritten(tmp_path, parent, edit))
    assert status == 1, err
    flagged = [n for n, line in enumerate(lines[:-1]) if line["not_slower_beyond_the_two_spreads"] is not True]
    assert flagged == [7] and lines[7]["not_slower_beyond_the_two_spreads"] is False
    assert lines[-1]["slower_beyond_the_two_spreads"] == 1 and lines[-1]["rows"] == 72


class RecordingContext:
    """What alternate() needs of a context: the timing section; every section takes the next of `times`."""

    def __init__(self, events, times):
        self.events, self.times = events, iter(times)

    def timing_begin(self):
        self.events.append("begin")

    def timing_end_ms(self):
        self.events.append("end")
        return next(self.times)


def test_alternate_order_of_work(bk):
    events = []
    ctx = RecordingContext(events, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    calls = {name: (lambda name=name: events.append(name)) for name in "abc"}
    calls["b"] = (calls["b"], bk.KERNEL)  # a bare callable and (call, KERNEL) are the same kind
    wall, kernel = bk.alternate(ctx, calls, 2, sync=lambda: events.append("sync"))
    timed = ["begin", "%s", "sync", "end"]
    assert events == ["a", "b", "c", "sync"] + [e % name if e == "%s" else e for name in "abcabc" for e in timed]
    assert kernel == {"a": [1.0, 4.0], "b": [2.0, 5.0], "c": [3.0, 6.0]}
    assert wall == {"a": [], "b": [], "c": []}


def test_alternate_refuses_a_negative_section_time(bk):
    ctx = RecordingContext([], [1.0, -1.0])
    with pytest.raises(RuntimeError, match="a timing section with too many launches"):
        bk.alternate(ctx, {"a": lambda: None, "b": lambda: None}, 1, sync=lambda: None)
    sectioned = lambda section: [section(lambda: None) for _ in range(2)]  # noqa: E731
    with pytest.raises(RuntimeError, match="a timing section with too many launches"):
        bk.alternate(RecordingContext([], [1.0, -1.0]), {"a": (sectioned, bk.SECTIONS)}, 1, sync=lambda: None)


def test_alternate_sums_the_sections_of_a_call(bk):
    events = []
    ctx = RecordingContext(events, [0.5, 0.25, 0.125, 1.0, 2.0, 4.0, 8.0, 16.0])

    def three_parts(section):
        for part in "xyz":
            section(lambda part=part: events.append(part))

    wall, kernel = bk.alternate(ctx, {"three": (three_parts, bk.SECTIONS), "one": lambda: events.append("one")}, 2, sync=lambda: None)
    assert kernel == {"three": [0.875, 14.0], "one": [1.0, 16.0]}
    assert events[:4] == ["x", "y", "z", "one"]  # the warm-up runs the parts outside a timing section
    assert events[4:] == 2 * (["begin", "x", "end", "begin", "y", "end", "begin", "z", "end"] + ["begin", "one", "end"])


def test_alternate_host_clock(bk):
    events = []
    ctx = RecordingContext(events, [1.5, 2.5])
    calls = {"both": (lambda: events.append("both"), bk.WALL_KERNEL), "wall": (lambda: events.append("wall"), bk.WALL)}
    wall, kernel = bk.alternate(ctx, calls, 1, sync=lambda: events.append("sync"))
    # a host-clock timing starts from a synchronised device; the kernel time is read behind the clock
    assert events == ["both", "wall", "sync", "sync", "begin", "both", "sync", "end", "sync", "wall", "sync"]
    assert kernel == {"both": [1.5], "wall": []}
    assert [len(wall["both"]), len(wall["wall"])] == [1, 1] and all(t >= 0 for t in wall["both"] + wall["wall"])


def test_stats_rate_and_criterion(bk):
    ts = [0.71234, 0.70006, 0.73338, 0.70998, 0.72004]
    assert bk.stats(ts) == {"kernel_ms": 0.7123, "kernel_ms_min": 0.7001, "kernel_ms_spread": 0.0333}
    assert bk.stats(ts[:4], "wall_ms") == {"wall_ms": 0.7112, "wall_ms_min": 0.7001, "wall_ms_spread": 0.0333}  # even: the mean of the middle two
    assert list(bk.stats(ts, "ms")) == ["ms", "ms_min", "ms_spread"]
    assert bk.PEAK_GBPS == 8000.0
    assert bk.rate(1000 * 10 ** 6, 0.3) == (3333.3, 0.417)  # 3333.33 GB/s; 3333.3 / 8000 = 0.41666
    assert bk.rate(8000 * 10 ** 6, 2.0) == (4000.0, 0.5)
    parent = {"kernel_ms_min": 1.0, "kernel_ms_spread": 0.5}  # (binary fractions: the sums are exact)
    assert bk.not_slower({"kernel_ms_min": 1.75, "kernel_ms_spread": 0.25}, parent) is True  # at the bound
    assert bk.not_slower({"kernel_ms_min": 1.751, "kernel_ms_spread": 0.25}, parent) is False
    assert bk.not_slower({"wall_ms_min": 0.9, "wall_ms_spread": 0.0}, {"wall_ms_min": 1.0, "wall_ms_spread": 0.0}, "wall_ms") is True
    assert bk.shape(["tool", "--small"]) == (360, 180, 24) and bk.shape(["tool"]) == (1440, 720, 137)
    assert bk.shape(["tool", "--small"], (8, 4), (2, 1)) == (2, 1)
