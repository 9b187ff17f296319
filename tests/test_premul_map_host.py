"""The hoisted first twiddle product of the forward 64-bit ring 2^16 (csrc/contig_p4_map.hpp: premul), no GPU:
tests/cpp/premul_map_check.cpp compiled for the HOST with AddressSanitizer and UBSan (a stand-alone program) walks every
tile of the strided K = 6 pass for mod_count 1 and 3 -- the multiplied positions are exactly those with ring bit 9 set,
each with the table slot the last pass reads today for the first stage of its segment -- and checks, in exact 128-bit
integers at the widest modulus of the 31 q and 16 q families, that U = cap q - 1 and T = 4 q - 1 keep both outputs of
the new first stage below LIMIT q and below 2^64."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multiplied_positions_are_the_bit_9_half_with_todays_table_slots_and_the_ranges_hold(tmp_path):
    exe = str(tmp_path / "premul_map_check")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gpu-ntt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "premul_map_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK ") and "WRONG" not in r.stdout
    # 32 polynomials x 65536 positions, several checks each
    assert int(r.stdout.split()[1]) > 4 * 32 * 65536
