"""What the lazy-arithmetic tests need from outside tests/lazy_model.py (which stays plain Python): the compiler for
tests/cpp/lazy_arith_probe.hip, and the library's host-side Modulus<T> / the NTT-prime search for the generator's moduli."""
import os
import subprocess

import lazy_model as L

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_probe(exe):
    """compile tests/cpp/lazy_arith_probe.hip for gfx950 (no GPU needed for that, nor for its host-only modes)"""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "lazy_arith_probe.hip")
    subprocess.check_call([HIPCC, "-x", "hip", src, "-O2", "-std=c++20", "--offload-arch=gfx950",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe], timeout=300)
    return exe


def library_hooks():
    """(bit_of, find_ntt_prime) for family_moduli: the library's own host-side Modulus<T> (it states `bit`, and refuses
    what the kernels cannot take) and the NTT-prime search of the GPU tests.  Host code only; no GPU is touched."""
    from conftest import load_pkg
    from gpu_utils import find_ntt_factors
    g = load_pkg()

    def bit_of(q, W):
        try:
            return g.Modulus(q, bits=W).bit
        except ValueError:
            return None

    def find_ntt_prime(b):
        for logn in range(min(b - 2, 12), -1, -1):
            try:
                return find_ntt_factors(b, logn, clear_of_top=True)[0]
            except ValueError:
                continue
        return None

    return bit_of, find_ntt_prime


_CASES = {}


def family_cases(name):
    """(moduli, Cases) of a family, generated once per process"""
    if name not in _CASES:
        fam = L.FAMILIES[name]
        moduli = L.family_moduli(fam, *library_hooks())
        _CASES[name] = (moduli, L.generate(fam, moduli))
    return _CASES[name]
