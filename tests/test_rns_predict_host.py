"""The family prediction of the drop-in RNS calls (csrc/rns_predict.hpp, the rules behind host::rns_guess), no GPU:
tests/cpp/rns_predict_check.cpp compiled for the HOST with AddressSanitizer and UBSan (a stand-alone program) plays the
device -- it writes into a slot's word what a finished call would publish -- and walks: a fresh moduli buffer per call
(the shape hint learns from finished calls in OTHER buffers), calls that have not finished, a hint that must not hide a
wider stack, narrowing after 16 observations, alternating stacks, shape isolation, out-of-domain stacks, LRU recycling of
the words, reset_predictions, and the per-slot rules (widen at once, narrow after 16, exact mode of the 4-step entry).
Two option-parsing rules of the same host code ride along (they need the library, not a GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ["fresh_buffer_per_call", "word_not_yet_written", "a_hint_does_not_hide_a_wider_stack", "narrowing",
             "alternating_stacks", "shape_isolation", "out_of_domain", "lru_recycling", "reset_predictions", "per_slot_rules"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rns_predict") / "rns_predict_check")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rns_predict_check.cpp"), "-o", out])
    return out


def test_every_scenario_of_the_prediction_rules(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK ") and "WRONG" not in r.stdout
    assert int(r.stdout.split()[1]) > 2000  # every scenario ran its loops


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario(exe, name):
    """one scenario at a time, so that a failure names it (the program stops at its first mismatch)"""
    r = subprocess.run([exe, name], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK ")


def test_the_program_knows_its_scenarios(exe):
    r = subprocess.run([exe, "no_such_scenario"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "WRONG" in r.stdout


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build_library()
    return pkg.load_library()


def test_reset_predictions_takes_the_value_1_only(lib):
    assert lib.gpuntt_test_set_hook(b"reset_predictions", b"1") == 0
    assert lib.gpuntt_test_set_hook(b"reset_predictions", b"0") != 0  # (was taken as a reset)
    assert lib.gpuntt_set_option(b"reset_predictions", b"1") != 0  # a test hook, not an option


def test_option_numbers_are_decimal(lib):
    """a leading zero is no octal prefix: "020" is twenty (baseconv_ksplit takes 0 .. 16; octal 020 = 16 would pass);
    masks may still be written in hexadecimal with 0x"""
    try:
        assert lib.gpuntt_test_set_hook(b"baseconv_ksplit", b"020") != 0
        assert lib.gpuntt_test_set_hook(b"baseconv_ksplit", b"016") == 0
        assert lib.gpuntt_test_set_hook(b"keyswitch_hoist_chunk", b"010") == 0  # ten; 6 .. 13
        assert lib.gpuntt_test_set_hook(b"keyswitch_hoist_chunk", b"014") != 0  # fourteen (octal: twelve)
        assert lib.gpuntt_set_option(b"rns_predict", b"01") == 0
        assert lib.gpuntt_test_set_hook(b"u32_e32", b"0xf000") == 0 and lib.gpuntt_test_set_hook(b"u32_e32", b"61440") == 0
        for bad in (b"0x", b"0xg", b"1 ", b" 1", b"+", b""):
            assert lib.gpuntt_test_set_hook(b"u32_e32", bad) != 0, bad
    finally:
        for name, value in ((b"baseconv_ksplit", b"0"), (b"keyswitch_hoist_chunk", b"0"), (b"u32_e32", b"0x1f000")):
            assert lib.gpuntt_test_set_hook(name, value) == 0
