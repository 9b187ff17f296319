"""The argument checks the pipeline calls of the RNS plans share (csrc/rns_call.hpp), no GPU: tests/cpp/rns_call_check.cpp
compiled for the HOST with AddressSanitizer and UBSan (a stand-alone program, a plain clang++, nothing preloaded) compares
the overlap refusal with a brute-force definition over every pair of small synthetic ranges -- adjacent, nested,
zero-length, identical with and without the "may be exactly this write" permission, the same start with another length --
and walks null operands, several writes against several reads, the message thrown and the pair that decides it, and the
alignment (255 / 256 / 257), int-batch (0x7FFFFFFF / 0x80000000), null-pointer and scratch-region helpers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ["every_small_pair", "named_cases", "null_operands", "lists_and_order", "alignment_and_batch",
             "pointers_and_regions"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rns_call") / "rns_call_check")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rns_call_check.cpp"), "-o", out])
    return out


def test_every_scenario(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK ") and "WRONG" not in r.stdout
    assert int(r.stdout.split()[1]) > 30000  # the exhaustive pairs ran


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario(exe, name):
    """one scenario at a time, so that a failure names it (the program stops at its first mismatch)"""
    r = subprocess.run([exe, name], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK ")


def test_the_program_knows_its_scenarios(exe):
    r = subprocess.run([exe, "no_such_scenario"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "WRONG" in r.stdout


def test_the_header_includes_nothing_of_hip():
    """a plain host compiler builds it: no HIP header, directly or through rns_host.hpp"""
    for name in ("rns_call.hpp", "rns_host.hpp"):
        with open(os.path.join(ROOT, "gpu-ntt_amd", "csrc", name)) as f:
            includes = [line.split()[1] for line in f if line.startswith("#include")]
        assert all("hip" not in inc for inc in includes), (name, includes)
        assert all(inc.startswith("<") or inc == '"rns_host.hpp"' for inc in includes), (name, includes)
