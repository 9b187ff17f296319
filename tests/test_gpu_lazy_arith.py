"""The lazy modular arithmetic of gpu-ntt_amd/csrc/lazy.hpp on the device, primitive by primitive, against exact integers.

tests/cpp/lazy_arith_probe.hip includes the header and runs every member a kernel calls -- mul / mul_acc / mul_acc_raw in
both twiddle forms (scalar and vector registers), mulc, csub<K>, csub_c<K>, shl1_add, reduce_2q, normalize<B>, xad_not --
for one family per run: the Mod<...> specialisations the library instantiates, uniform and per-lane moduli.  The operands
(tests/lazy_model.py) put lazy values on the edges of their ranges for moduli of every width the family takes: k q + {-2
.. 2}, the top of the word, products whose dropped-partial-product quotient is two short and reach 3 q (that they do is
checked on the CPU, tests/test_lazy_model_host.py).  EVERY result word is compared with its contract."""
import subprocess

import pytest

import lazy_model as L
import lazy_probe_utils as U

pytestmark = pytest.mark.gpu

# set when a probe run ended on a signal or at its time limit: nothing more is started on the device by this module
_dead = []


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return U.build_probe(str(tmp_path_factory.mktemp("lazy_probe") / "lazy_arith_probe"))


def run_probe(exe, case_file, out_file):
    if _dead:
        pytest.fail("not started: an earlier probe run %s" % _dead[0])
    try:
        r = subprocess.run([exe, "run", case_file, out_file], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _dead.append("hit its time limit")
        pytest.fail("the probe hit its time limit")
    if r.returncode < 0:
        _dead.append("ended on signal %d" % -r.returncode)
    elif r.returncode == 3:  # a HIP call failed (the probe's HIP_CHECK): a fault shows up that way too
        _dead.append("ended on a HIP error: " + r.stderr.strip()[-300:])
    assert r.returncode == 0, "probe exit %d\n%s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("family", list(L.FAMILIES))
def test_every_primitive_meets_its_contract(probe, tmp_path, family):
    moduli, cases = U.family_cases(family)
    assert cases.ncase <= L.MAX_CASES
    case_file, out_file = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    L.write_cases(cases, case_file)
    run_probe(probe, case_file, out_file)
    fails = L.verify(cases, L.read_results(out_file, cases.fam, cases.ncase))
    assert not fails, "\n".join(fails[:20])
