"""The host twin of the Gram coordinate-descent solver (csrc/runtime/enet_cpu.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer: ``csrc/tests/enet_selftest.cpp`` is built with
``-fsanitize=address,undefined -fno-sanitize-recover=all`` and run as a plain executable (d = 1,
d = 65, an all-zero Gram, max_iter = 1, positive, F = 0, interleaved Grams), each result checked
against a straight scalar loop inside the program."""
import os
import shutil
import subprocess

import pytest

from cs230_distributed_machine_learning_amd import build


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_enet_twin_clean_under_asan_ubsan():
    exe = build.build_enet_selftest()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", OMP_NUM_THREADS="4")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "enet_selftest: ok" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
