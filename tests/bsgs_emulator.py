"""Shared by tests/test_bsgs_host.py: cut the kern namespace out of csrc/hoisted_rotation.hip, build
tests/cpp/emulate_bsgs.cpp around it for the HOST with AddressSanitizer and UBSan (a stand-alone program, one thread per
lane; a plain clang++, nothing preloaded) and run it for one kernel of linear_transform_bsgs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_emulator(tmp_path, which):
    """which: "scale" (bsgs_scale_input), "sum" (bsgs_weighted_sum) or "giant" (inner_product_galois_giant); asserts that
    the program ends with ALL OK and returns what it printed"""
    text = open(os.path.join(ROOT, "gpu-ntt_amd", "csrc", "hoisted_rotation.hip")).read()
    first, last = text.index("        constexpr int HOIST_NT"), text.index("    } // namespace kern")
    (tmp_path / "kernel_extract.inc").write_text(text[first:last])
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "emulate_bsgs")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(cpp, "host_shim"),
                           "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(cpp, "emulate_bsgs.cpp"), "-o", exe], timeout=300)
    r = subprocess.run([exe, which], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout
