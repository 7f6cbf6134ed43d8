"""What Engine (ma_amd/host/ma_engine.h) asks of the C ABI, call by call, on the CPU: tests/emul/engine_calls_test.cpp stubs every
symbol the engine reaches, prints each call with its value arguments and, after every scenario, the scalar fields of the result.
tests/golden/engine_calls.txt is that output as the header produced it before its run bodies were folded into one; it is not
regenerated: a change of the header that alters a call, its order or its arguments shows up as the first differing line."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "engine_calls_test.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_calls.txt")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
STDERR_MARK = "---- stderr, pointer and numbers masked ----\n"


def _output(cmd, tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.check_call(cmd + ["-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-pthread"])
    env = {k: v for k, v in os.environ.items() if k != "MA_ENGINE_TRACE"}
    p = subprocess.run([exe], env=dict(env, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    err = re.sub(r"engine 0x[0-9a-f]+", "engine PTR", p.stderr)
    err = re.sub(r"(?<![a-z])\d+(\.\d+)?", "N", err)  # (every decimal number; the digit of "h2d" and "d2h" is a letter here)
    return p.stdout + STDERR_MARK + err


def _compare(got):
    want = open(GOLDEN).read()
    g, w = got.splitlines(), want.splitlines()
    for i, (a, b) in enumerate(zip(g, w)):
        assert a == b, "line %d differs:\n  got:    %s\n  golden: %s" % (i + 1, a, b)
    assert len(g) == len(w), "%d lines, the golden has %d; first extra line: %s" % (len(g), len(w), (g + w)[min(len(g), len(w))])
    assert got == want


def test_engine_calls_match_the_golden_trace(tmp_path):
    """run (plain, stages, SoC queues, pairs, SAM with all / no / some qualities, paired SAM; each with and without inversions),
    runText (fits, capacity retry, refusal), runBgzf, runMatesText (fits, retry, refusal), recycled results and the
    MA_ENGINE_TRACE lines: the calls, their order, their arguments and the results' scalars are those of the golden."""
    _compare(_output(["g++", "-std=c++17", "-O1", "-Wall"], tmp_path, "engine_calls_test"))


def test_engine_calls_under_sanitizers(tmp_path):
    """The same stand-alone program under -fsanitize=address,undefined: the stubs fill every array as the library would, so an
    array the engine sized too small, a read of a freed result or a leaked batch is a report.  Same output."""
    if not os.path.exists(CLANG):
        pytest.skip("no clang")
    got = _output([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-w"], tmp_path, "engine_calls_test_san")
    assert "runtime error" not in got and "Sanitizer" not in got, got[-2000:]
    _compare(got)
