"""CPU test of csrc/fps_plan.h, the rule by which afm_fps picks its kernel and launch shape: a stand-alone C program prints the plan of every
n in 1 ... 16500 for m in {1, 31, 32, n}; every line is compared with `parent_plan` below, a restatement of the if / else ladder afm_fps held
before the rule moved into the header (commit 7fa6b6e), written from that function and not from the header.  No kernel is launched."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

N_MAX = 16500
LDS_LIMIT = 150 * 1024
# (form, PPT): every kernel the library instantiates, and nothing else
ARMS = {("pruned", 2), ("pruned", 4), ("pruned", 8), ("lds", 1), ("lds", 2), ("lds", 4), ("lds", 8), ("lds", 16), ("lds", 32), ("global", 32)}
PLAIN_EDGES = [64, 128, 256, 512, 1024, 12800, 16384]              # the arm changes between n and n + 1, whatever m is
PRUNED_EDGES = [1535, 2048, 4096, 8192]                            # ... and where m >= 32

PROGRAM = r"""
#include <stdio.h>
#include "fps_plan.h"
int main(void) {
    static const char* form[] = {"unsupported", "pruned", "lds", "global"};
    for (int n = 1; n <= %d; ++n) {
        const int ms[4] = {1, 31, 32, n};
        for (int i = 0; i < 4; ++i) {
            const FpsPlan p = fps_plan(n, ms[i]);
            printf("%%d %%d %%s %%d %%d %%d\n", n, ms[i], form[p.form], p.ppt, p.threads, p.lds_bytes);
        }
    }
    return 0;
}
""" % N_MAX


def parent_plan(n, m):
    """afm_fps of the parent commit, line by line: -> (form, PPT, threads, dynamic LDS bytes)."""
    np2 = 2048
    while np2 < n:
        np2 <<= 1
    if n >= 1536 and np2 <= 8192 and m >= 32:                      # `prune`; PT = 1024, kernel <np2 / PT, PT>
        return ("pruned", np2 // 1024, 1024, max(3 * n, 2 * np2) * 4)
    T = (((n + 31) // 32 + 63) // 64) * 64
    T = max(T, 64)
    T = min(T, 512)
    if (n + T - 1) // T > 32:
        T = 1024
    ppt = (n + T - 1) // T
    lds = 3 * n * 4
    in_lds = lds <= 150 * 1024
    if T <= 512 and 16 < ppt <= 32:
        P = 32
    elif ppt <= 1:
        P = 1
    elif ppt <= 2:
        P = 2
    elif ppt <= 4:
        P = 4
    elif ppt <= 8:
        P = 8
    elif ppt <= 16:
        P = 16
    else:
        return ("unsupported", 0, 0, 0)
    return ("lds", P, T, lds) if in_lds else ("global", P, T, 0)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    d = tmp_path_factory.mktemp("fps_plan")
    src, exe = d / "plan.c", d / "plan"
    src.write_text(PROGRAM)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "afford-motion_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        n, m, form, ppt, threads, lds = line.split()
        out[(int(n), int(m))] = (form, int(ppt), int(threads), int(lds))
    assert set(out) == {(n, m) for n in range(1, N_MAX + 1) for m in (1, 31, 32, n)}
    return out


def test_every_plan_is_the_parents(plans):
    wrong = [(k, got, parent_plan(*k)) for k, got in plans.items() if got != parent_plan(*k)]
    assert not wrong, wrong[:5]
    for (n, m), (form, ppt, threads, lds) in plans.items():        # (named on their own: the launch shape)
        assert threads == parent_plan(n, m)[2] and threads <= 1024 and threads % 64 == 0
        assert lds <= LDS_LIMIT
        assert form == "unsupported" or threads * ppt >= n         # every point has a slot


def test_exactly_the_instantiated_kernels_occur(plans):
    arms = {p[:2] for p in plans.values() if p[0] != "unsupported"}
    assert arms == ARMS
    assert {n for (n, m), p in plans.items() if p[0] == "unsupported"} == set(range(16385, N_MAX + 1))
    assert {n for (n, m), p in plans.items() if p[0] == "global"} == set(range(12801, 16385))      # 12 n > 150 KB


def test_arm_boundaries(plans):
    def edges(m_of):
        return [n for n in range(1, N_MAX) if plans[(n, m_of(n))][:2] != plans[(n + 1, m_of(n + 1))][:2]]
    assert edges(lambda n: 1) == PLAIN_EDGES and edges(lambda n: 31) == PLAIN_EDGES
    assert edges(lambda n: 32) == sorted(PLAIN_EDGES + PRUNED_EDGES) == edges(lambda n: n)
    assert plans[(1536, 31)][:2] == ("lds", 32) and plans[(1536, 32)][:2] == ("pruned", 2)
    assert plans[(1535, 32)][:2] == ("lds", 32) and plans[(8193, 32)][:2] == ("lds", 32)
    assert [plans[(n, 32)][:2] for n in (2048, 2049, 4096, 4097, 8192)] == [("pruned", 2), ("pruned", 4), ("pruned", 4), ("pruned", 8), ("pruned", 8)]
    assert [plans[(n, 1)][:2] for n in (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 12800, 12801, 16384)] == [
        ("lds", 1), ("lds", 2), ("lds", 2), ("lds", 4), ("lds", 4), ("lds", 8), ("lds", 8), ("lds", 16), ("lds", 16), ("lds", 32), ("lds", 32),
        ("global", 32), ("global", 32)]
