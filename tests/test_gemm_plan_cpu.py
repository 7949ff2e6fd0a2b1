"""The bf16 GEMM dispatch, pinned on the CPU: which kernel family, tile, split-K and sub-variant every
problem lands on, the refusals, and what the planning queries answer.

``tests/gemm_plan_dump.hip`` includes ``csrc/gemm.hip`` with the kernel launches stubbed out, calls the C entry
points over the presets' layer shapes, the GPU tests' case tables and a seeded sweep of 20 000 problems, and
prints return codes, launch records and queries.  ``tests/golden/gemm_plan_parent.txt`` is that output as
recorded on the commit before the dispatch was rewritten around one plan function (``csrc/gemm_plan.h``); it is
never regenerated from later code: a difference here means a problem changed kernels, not that the file is stale.
Each knob that moves the plan gets a run of its own, in a child process (the knobs are read once per process).
"""
import os
import subprocess

import pytest

from distributed_training_compare_jax_amd.csrc import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gemm_plan_dump.hip")
GOLDEN = os.path.join(HERE, "golden", "gemm_plan_parent.txt")

# (environment, listing mode): the default plan with one line per featured shape, each knob as digests only
RUNS = [({}, "brief")] + [({k: v}, "digest") for k, v in (
    ("DTC_GEMM_W8", "2"), ("DTC_GEMM_W8", "0"), ("DTC_GEMM256", "0"), ("DTC_GEMM_DMA", "0"), ("DTC_GEMM8R", "7"),
    ("DTC_GEMM8N", "7"), ("DTC_WGRAD256", "0"), ("DTC_WGRAD_BLOCKS", "128"))]


def _compile(out, *defines):
    cmd = [B.hipcc(), f"--offload-arch={B.ARCH}", "--cuda-host-only", "-O1", "-std=c++17", "-w", *defines,
           "-I", B.HERE, SRC, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _label(env):
    return " ".join(f"{k}={v}" for k, v in env.items()) or "default knobs"


def _run(exe, env, mode):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DTC_")}
    r = subprocess.run([exe, mode], env={**clean, **env}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{_label(env)}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
    return f"## {_label(env)}\n{r.stdout}"


def _golden_sections():
    with open(GOLDEN) as f:
        parts = f.read().split("## ")
    return {p.split("\n", 1)[0]: "## " + p for p in parts[1:]}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump"))


@pytest.fixture(scope="module")
def exe_check(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("gemm_plan_check") / "gemm_plan_dump"), "-DPLAN_CHECK")


def _first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return f"line {i + 1}:\n  now:    {a}\n  parent: {b}"
    return f"length: {len(g)} lines now, {len(w)} on the parent"


@pytest.mark.parametrize("env,mode", RUNS, ids=[_label(e).replace(" ", "_") for e, _ in RUNS])
def test_plan_table_matches_parent(exe, env, mode):
    got, want = _run(exe, env, mode), _golden_sections()[_label(env)]
    assert got == want, _first_difference(got, want)


@pytest.mark.parametrize("env,mode", RUNS, ids=[_label(e).replace(" ", "_") for e, _ in RUNS])
def test_plan_query_is_what_launches(exe_check, env, mode):
    """dtc_gemm_plan returns, for every row of the table and the sweep, exactly the return code and the launch
    record of dtc_gemm (the harness exits 3 at the first row where they differ), and launches nothing."""
    got, want = _run(exe_check, env, mode), _golden_sections()[_label(env)]
    assert got == want, _first_difference(got, want)
