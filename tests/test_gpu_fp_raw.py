"""GPU twin of test_host_sim_fp_raw.py: the Fp / Fp2 leaf routines on RAW limbs at the documented bounds, one lane per element, through
fp_raw_kernel — an entry that only the experiments library exports (c12381_exp_fp_raw_batch), loaded the way test_gpu_variants.py loads
it (child process, C12381_LIB).  The operands the product entries can reach are normalised by fp_from_words_be; here the kernel sees
negative limbs, limbs at +-L(T) and 2^31 - 1, values from -20000 p to 20000 p and non-zero multiples of p.  Every raw output limb is
compared with the integer the mathematics predicts (fp_raw_vectors.py: the same vectors and expectations as on the host, so host ==
device follows), in batches of 1, 63, 65 elements and the whole set; the closure run alternates lazy operations and products for a
few thousand launches.  Vectors per op: fp_raw_vectors.COUNTS, all of them run.

The family "Fp2, two lanes" runs csrc/fp2h.hpp in its DEVICE form through fp2h_raw_kernel (the same entry, by op code): two adjacent lanes
per element, each holding one half, the partner's half fetched by DPP and the role taken from the lane number — code the host simulation
cannot execute.  Both halves of every result are compared, and the first 1, 31, 32, 33 elements are run again on their own (2, 62, 64, 66
lanes: a lone pair, a pair that ends a wavefront, a wavefront plus one pair)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "crypto12381_amd", "lib", "libc12381_hip_exp.so")

CODE = r"""
import sys
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import tools.libsel  # C12381_LIB -> capi.use_library
import fp_raw_vectors as V
from crypto12381_amd import Context
c = Context(0)

def run(name, vecs):
    limbs, _, k = V.pack(name, vecs)
    return V.unpack(name, c.exp_fp_raw(V.OPS[name], len(vecs), V.ARITY[name], V.OUTPUTS[name], limbs, k), len(vecs))

mode = sys.argv[1]
if mode == 'family':
    for name in V.FAMILIES[sys.argv[2]]:
        vecs = V.vectors(name)
        assert len(vecs) == V.COUNTS[name]
        outs = run(name, vecs)
        bad = []
        for i, (v, o) in enumerate(zip(vecs, outs)):
            try:
                V.check_outputs(name, v, o)
            except AssertionError as e:
                bad.append('lane %d: %s' % (i, e))
        assert not bad, '%s: %d of %d lanes differ\n%s' % (name, len(bad), len(vecs), '\n'.join(bad[:4]))
        # batch sizes off the wavefront / block size: same lanes, same limbs (two lanes per element in the two-lane family)
        for n in ((1, 31, 32, 33) if name[:4] == 'FH2_' else (1, 63, 65)):
            assert run(name, vecs[:n]) == outs[:n], (name, n)
        print('%s: %d vectors' % (name, len(vecs)))
else:
    kinds = (V.closure if mode == 'closure' else V.closure_fp2h)(run, 3000)
    assert sum(kinds.values()) == 3000
    print('closure steps:', kinds)
c.close()
print('fp raw ok')
"""


def child(*args):
    e = dict(os.environ)
    for k in [k for k in e if k.startswith("C12381_")]:
        del e[k]
    e["C12381_LIB"] = EXP_LIB
    r = subprocess.run([sys.executable, "-c", CODE, *args], env=e, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "fp raw ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


@pytest.mark.parametrize("family", ["product + reduction", "injected reductions", "exact carries", "canonical form and predicates", "Fp2", "doubling and psi forms", "Fp2, two lanes"])
def test_raw_limbs_at_the_bounds(family):
    child("family", family)


def test_closure_lazy_ops_between_products():
    child("closure")


def test_closure_two_lane_fp2_as_the_g2_formulas_mix_them():
    child("closure_fp2h")


def test_product_library_has_no_raw_entry():
    from crypto12381_amd import Context
    c = Context(0)
    assert not hasattr(c.lib, "c12381_exp_fp_raw_batch")
    with pytest.raises(RuntimeError):
        c.exp_fp_raw(0, 1, 2, 1, bytes(112), bytes(16))
    c.close()
