"""Index maps of the four-polynomial tile of the forward 64-bit contiguous pass (csrc/contig_p4_map.hpp), no GPU:
tests/cpp/contig_p4_map_check.cpp compiled for the HOST with AddressSanitizer and UBSan (a stand-alone program) walks
every round's thread -> tile element map (a bijection on the 4096 elements), the LDS slots, the memory offsets and, for
every lane, register and segment, the twiddle index against the one-polynomial tile's index for the same ring position."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_maps_are_bijections_and_the_twiddle_indices_are_the_one_polynomial_tiles(tmp_path):
    exe = str(tmp_path / "contig_p4_map_check")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "contig_p4_map_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK ") and "WRONG" not in r.stdout
    assert int(r.stdout.split()[1]) > 1000000  # every lane, register, stage and segment was visited
