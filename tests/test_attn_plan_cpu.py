"""The bf16 attention dispatch, pinned on the CPU: which kernels every problem launches, in which order, on which
grid, block and dynamic LDS size, with which block order, and the refusals.

``tests/attn_plan_dump.hip`` includes ``csrc/attention.hip`` with the kernel launches replaced by a call that
writes down the kernel expression and the geometry, calls ``dtc_attn_fwd`` / ``dtc_attn_bwd`` over the shapes of
the GPU tests, a grid of (T, B, H, head_dim), every flag value and a seeded sweep of 6000 problems, and prints
return codes and launches.

``tests/golden/attn_plan_parent.txt`` is that output as recorded on commit e5f852e, the last one whose
``attention.hip`` chose its kernels in if-ladders at the end of the file, before ``csrc/attn_plan.h`` existed: the
same program built with ``-DATTN_PLAN_PARENT`` (the text then comes from the launch macro alone) by an ordinary
``hipcc --offload-arch=gfx950 -O1`` compile, run once per section below.  It is never regenerated from later
code: a difference here means a problem changed kernels, not that the file is stale.  Each knob gets a run of its
own, in a child process (the knobs are read once per process), and so does each CU count: 256 (the MI355X),
304 and 64 (the balanced block order appears on other grids) and 0 (the device query failed).
"""
import os
import re
import shutil
import subprocess

import pytest

from distributed_training_compare_jax_amd.csrc import build as B
from distributed_training_compare_jax_amd.ops import attention as A

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "attn_plan_dump.hip")
ORDER_SRC = os.path.join(HERE, "native", "attn_order_check.cpp")
GOLDEN = os.path.join(HERE, "golden", "attn_plan_parent.txt")

# (section label, environment, listing mode, CU count)
RUNS = [("default knobs", {}, "brief", 256)] + [
    (" ".join(f"{k}={v}" for k, v in env.items()), env, "digest", 256) for env in (
        {"DTC_ATTN_RESIDENT": "0"}, {"DTC_ATTN_CHUNK": "0"}, {"DTC_ATTN_FUSED": "0"},
        {"DTC_ATTN_FUSED": "0", "DTC_ATTN_MERGED": "0"}, {"DTC_ATTN_BWD_MERGED": "0"})] + [
    (f"{cus} CUs", {}, "digest", cus) for cus in (304, 64, 0)]
IDS = [r[0].replace(" ", "_") for r in RUNS]


def _compile(out, *defines):
    cmd = [B.hipcc(), f"--offload-arch={B.ARCH}", "--cuda-host-only", "-O1", "-std=c++17", "-w", *defines,
           "-I", B.HERE, SRC, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(exe, label, env, mode, cus):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DTC_")}
    r = subprocess.run([exe, mode, str(cus)], env={**clean, **env}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{label}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
    return f"## {label}\n{r.stdout}"


def _golden_sections():
    with open(GOLDEN) as f:
        parts = f.read().split("## ")
    return {p.split("\n", 1)[0]: "## " + p for p in parts[1:]}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("attn_plan") / "attn_plan_dump"))


@pytest.fixture(scope="module")
def exe_check(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("attn_plan_check") / "attn_plan_dump"), "-DPLAN_CHECK")


def _first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return f"line {i + 1}:\n  now:    {a}\n  parent: {b}"
    return f"length: {len(g)} lines now, {len(w)} on the parent"


@pytest.mark.parametrize("label,env,mode,cus", RUNS, ids=IDS)
def test_launches_match_parent(exe, label, env, mode, cus):
    """The text comes from dtc_attn_last_launch; the harness exits 3 at the first row whose record is not what
    the launch sites did (kernel expression, grid, block, LDS bytes, LDS opt-in, block order)."""
    got, want = _run(exe, label, env, mode, cus), _golden_sections()[label]
    assert got == want, _first_difference(got, want)


@pytest.mark.parametrize("label,env,mode,cus", RUNS, ids=IDS)
def test_plan_query_is_what_launches(exe_check, label, env, mode, cus):
    """dtc_attn_plan returns, for every row, exactly the return code and the record of the call itself (the
    harness exits 3 at the first row where they differ), and launches nothing."""
    got, want = _run(exe_check, label, env, mode, cus), _golden_sections()[label]
    assert got == want, _first_difference(got, want)


def test_python_name_tables_mirror_the_header():
    """ops/attention.py's KERNELS, PATHS and flag values are the header's, entry for entry."""
    with open(os.path.join(B.HERE, "attn_plan.h")) as f:
        h = f.read()
    names = re.search(r"KERNEL_NAMES\[\] = \{(.*?)\};", h, re.S).group(1)
    assert tuple(re.findall(r'"([^"]+)"', names)) == A.KERNELS
    paths = re.search(r"enum Path \{(.*?)PATH_COUNT", h, re.S).group(1)
    paths = [p.lower() for p in re.findall(r"^\s*([A-Z0-9_]+)\b", paths, re.M)]
    assert tuple("none" if p == "path_none" else p for p in paths) == A.PATHS
    for cls, prefix in ((A.FwdFlags, "FWD_"), (A.BwdFlags, "BWD_")):
        for flag in cls:
            bit = re.search(rf"\b{prefix}{flag.name} = 1 << (\d+)", h)
            assert bit and 1 << int(bit.group(1)) == flag.value, flag
    assert A.REC_INTS == 5 + 4 * int(re.search(r"MAX_LAUNCHES = (\d+)", h).group(1))


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")


def _order_check(tmp_path, *flags):
    exe = str(tmp_path / "attn_order_check")
    r = subprocess.run([_cxx(), "-O1", "-g", "-std=c++17", *flags, "-I", B.HERE, ORDER_SRC, "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and flags and "asan" in (r.stderr or "").lower():
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("ok"), run.stdout[-1000:]


@pytest.mark.skipif(_cxx() is None, reason="no host C++ compiler")
def test_fw_order_properties(tmp_path):
    """csrc/attn_plan.h compiles with a plain C++ compiler, and the balanced order is a bijection with exactly wps
    blocks per CU and CU loads within one heaviest block of each other wherever n > 0, and n == 0 wherever the
    one-round precondition fails (tests/native/attn_order_check.cpp)."""
    _order_check(tmp_path)


@pytest.mark.skipif(_cxx() is None, reason="no host C++ compiler")
def test_fw_order_asan_ubsan(tmp_path):
    """The same program under AddressSanitizer + UndefinedBehaviorSanitizer, as its own process: the indices
    fw_order computes into its fixed arrays stay in bounds over the whole sweep."""
    _order_check(tmp_path, "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
