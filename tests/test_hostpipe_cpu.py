"""The host-memory level pipeline (csrc/mifc_hostpipe.hip) without a GPU: its chunking policy through
mifc_host_chunk_levels, and its copy threads (csrc/mifc_copypool.h) in a stand-alone host program.  The same program runs
under the thread and the address sanitizers through `make -C mi-fieldcalc_amd copypool-check` (by hand, on the CPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mi-fieldcalc_amd", "libmifc.so")


@pytest.fixture(scope="module")
def policy():
    """mifc_host_chunk_levels under the DEFAULT policy.  The library reads its environment into a snapshot when a context is
    created or reloaded, never per call; without a context the snapshot holds the defaults whatever the environment says
    (and the tests that set the pipeline's switches restore the environment and have it re-read)."""
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    import mi_fieldcalc_amd._capi as capi

    fn = capi.lib().mifc_host_chunk_levels
    return lambda n, nlev: int(fn(int(n), int(nlev)))


@pytest.mark.parametrize("n,nlev,expected", [
    (1440 * 720, 16, 0),   # 66.36 MB < 64 MiB = 67.11 MB
    (1440 * 720, 17, 4),   # 32 MiB hold 8 levels, capped by nlev / 4
    (1440 * 720, 18, 4),   # test_hlevel_derived_levels_host_pipeline: 5 chunks
    (1440 * 720, 21, 5),   # test_vortdiv_levels_host_pipeline: 5 chunks
    (1440 * 720, 137, 8),  # 32 MiB / 4.15 MB
    (4000 * 4000, 1, 0),   # 64 MB < 64 MiB
    (4000 * 4000, 2, 1),   # a field larger than a chunk: one level at a time
    (4000 * 4000, 3, 1),
    (0, 1, 0), (0, 137, 0), (0, 1 << 20, 0),
    (1440 * 720, 0, 0),
])
def test_default_chunk_policy(policy, n, nlev, expected):
    assert policy(n, nlev) == expected


def test_default_chunk_policy_bounds(policy):
    """Either a batch is staged whole or 1 <= L <= max(1, nlev / 4); nothing below 64 MiB per field is pipelined."""
    sizes = [1, 4, 64 * 12, 260 * 9, 1440 * 92, 1440 * 720, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 4000 * 4000, 1 << 26, 1 << 28, (1 << 31) + 5]
    levels = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 64, 137, 1000, 65536]
    piped = 0
    for n in sizes:
        for nlev in levels:
            L = policy(n, nlev)
            if 4 * n * nlev < (64 << 20):
                assert L == 0, (n, nlev, L)
            else:
                piped += 1
                assert 1 <= L <= max(1, nlev // 4), (n, nlev, L)
                assert L * 4 * n <= (32 << 20) or L == 1, (n, nlev, L)
    assert piped > 50


def test_copy_pool_host_program(tmp_path):
    """tests/host/copypool_main.cc: pools of 1, 2 and 4 threads, two callers at once, sizes around the 2 MiB slice, guard
    bytes around every buffer, the pool destroyed while idle.  Plain g++, no HIP."""
    exe = tmp_path / "copypool"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "mi-fieldcalc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "copypool_main.cc"), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert res.stdout.startswith("copypool ok")
