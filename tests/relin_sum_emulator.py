"""For tests/test_relin_sum_host.py: cut the kern namespace out of csrc/relinearize_sum.hip, build
tests/cpp/emulate_relin_sum.cpp around it for the HOST with AddressSanitizer and UBSan (a stand-alone program, one thread
per lane; a plain clang++, nothing preloaded) and run it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_sum_emulator(tmp_path):
    """asserts that the program ends with ALL OK and returns what it printed"""
    text = open(os.path.join(ROOT, "gpu-ntt_amd", "csrc", "relinearize_sum.hip")).read()
    first = text.index("        // How inner_product_tensor_sum seeds")
    last = text.index("    } // namespace kern")
    (tmp_path / "kernel_extract.inc").write_text(text[first:last])
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "emulate_relin_sum")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(cpp, "host_shim"),
                           "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(cpp, "emulate_relin_sum.cpp"), "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout
