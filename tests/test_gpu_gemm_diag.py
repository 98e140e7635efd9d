"""The GEMM routes of the diagnostic library (nt_diag_route and the live tune keys of csrc/gemm.hip), element by element, with the bounds
of tests/gemm_check.py.

The product library holds none of this code, so the module starts ONE child Python process with LDMAE_HIP_LIB pointing at
libldmae_hip_diag.so; the child runs every case of CASES and prints one result line per case, the tests below each look one up.  A case
is run_nt / run_tn of test_gpu_gemm_paths.py on one shape, first with every tune key 0 (the shipped behaviour, once per shape) and then
with the case's keys set: NaN-padded Canvas operands and outputs, every element against the f64 reference, every canary, a bitwise
rerun and the launch count -- all as in that module.  Where the source says a variant computes the same products in the same order
(`bitwise`), every output must also equal the shipped kernel's bit for bit.  Every key is reset to 0 between cases.

  whole-line -> half-line kernel (key 19), per-K-step stamp build (7, bias and SwiGLU only), one tile per workgroup (8 = 2):
      M = 2056, N = 264, K = 192 -- nine row-blocks (persistent mapping, grid != ntiles), a ragged row tile and a ragged column tile;
      bias and SwiGLU-backward (Hs = 264).  Bitwise.
  start delay (5) and column-group walk (16 = 2 at N = 512: two column tiles) act on gemm_nt_persist_kernel only, so these cases pass
      LDMAE_EPI_HALF_LINES in both runs.  Bitwise.
  the 128 x 128 TN kernel (1) and a split target of 8 (9) at M = 4096, N = 264, K = 264 with the bias gradient: other orders of
      summation, so the per-element bound and the bitwise rerun only.

That a case's key takes its route rests on READING the predicates of nt_diag_route and launch_nt against the shapes above (stamps: the
epilogues it lists), not on the test: a route that refuses a shape falls through to the shipped kernel silently, with the same launch
count, and then passes the bitwise comparison trivially.  A key that nothing reads can no longer do so: ldmae_tune refuses every key
outside the live set of core.hip (tests/test_host_api.py), and the child asserts that each ldmae_tune call succeeds.

Key 11 (launch-gap probes: an empty kernel, or ntiles = 0) gives wrong results by design and is never set.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "ldmae_amd", "libldmae_hip_diag.so")

BIAS, GATE_RES, SWIGLU, SWIGLU_BWD, HALF = 0, 1, 4, 5, 0x200
# the shapes (case dicts of test_gpu_gemm_paths.py; dtype names resolved in the child)
SHAPES = {
    "bias": dict(kind="nt", M=2056, N=264, K=192, epi=BIAS),
    "swiglu_bwd": dict(kind="nt", M=2056, N=264, K=192, epi=SWIGLU_BWD),
    "bias_half": dict(kind="nt", M=2056, N=264, K=192, epi=BIAS, flags=HALF),
    "gate": dict(kind="nt", M=2048, N=512, K=768, epi=GATE_RES, rpb=256, gate="ld"),
    "gate_half": dict(kind="nt", M=2048, N=512, K=768, epi=GATE_RES, rpb=256, gate="ld", flags=HALF),
    "swiglu": dict(kind="nt", M=2048, N=512, K=512, epi=SWIGLU),
    "tn": dict(kind="tn", M=4096, N=264, K=264, bias=True),
}


def _case_table():
    cs = []

    def add(name, shape, keys, bitwise):
        cs.append(dict(name=f"{name}_{shape}", shape=shape, keys=keys, bitwise=bitwise))

    for shape in ("bias", "swiglu_bwd"):
        add("half_lines_key19", shape, [(19, 1)], True)
    for shape in ("bias", "swiglu"):
        add("stamps_key7", shape, [(7, 1)], True)
    add("delay_key5", "bias_half", [(5, 3)], True)
    add("colgroup_key16", "gate_half", [(16, 2)], True)
    for shape in ("bias", "gate"):
        add("tile_launch_key8", shape, [(8, 2)], True)
    for name, keys in (("tn_128_key1", [(1, 1)]), ("tn_target_key9", [(9, 8)])):
        add(name, "tn", keys, False)
    return cs


CASES = _case_table()
KEYS = (1, 5, 7, 8, 9, 16, 19)


# ----------------------------------------------------------------------------- the child process
def _child():
    import torch

    sys.path.insert(0, ROOT)
    import test_gpu_gemm_paths as gp
    from ldmae_amd import _lib

    lib = _lib.load()
    assert lib.ldmae_arch() == b"gfx950" and hasattr(lib, "ldmae_tune"), "the child needs the diagnostic library"
    defaults = {}

    def run(shape):
        """One case of test_gpu_gemm_paths.py -> (its outputs, worst |got - ref| / bound per output)"""
        c = dict(SHAPES[shape], name="diag_" + shape, dtype=gp.BF16, out=gp.BF16)
        outs = {}
        gp.RATIOS.clear()
        (gp.run_nt if c["kind"] == "nt" else gp.run_tn)(_lib, c, keep=outs)
        return outs, {k: round(v, 6) for k, v in gp.RATIOS.items()}

    fatal = None
    for c in CASES:
        res = {"name": c["name"], "ok": True, "msg": ""}
        try:
            assert all(lib.ldmae_tune_query(k) == 0 for k in KEYS)
            if c["shape"] not in defaults:                              # the shipped behaviour of the diagnostic build, once per shape
                defaults[c["shape"]] = run(c["shape"])
            res["default"] = defaults[c["shape"]][1]
            for k, v in c["keys"]:
                assert lib.ldmae_tune(k, v) == 0, f"{c['name']}: {_lib.last_error()}"
            outs, res["variant"] = run(c["shape"])
            assert outs and outs.keys() == defaults[c["shape"]][0].keys(), f"{c['name']}: outputs {sorted(outs)} to compare with {sorted(defaults[c['shape']][0])}"
            if c["bitwise"]:
                for n, t in defaults[c["shape"]][0].items():
                    it = gp._BITS[t.dtype][0]
                    assert torch.equal(t.view(it), outs[n].view(it)), f"{c['name']}: {n} is not bitwise equal to the shipped kernel's"
        except AssertionError as e:                                     # (BoundError included) a wrong result: go on with the next case
            res["ok"], res["msg"] = False, f"{type(e).__name__}: {e}"
        except Exception as e:                                          # a HIP error or a refused call: start nothing more on this device
            res["ok"], res["msg"] = False, f"{type(e).__name__}: {e}"
            fatal = res["msg"]
        for k in KEYS:
            lib.ldmae_tune(k, 0)
        print("RESULT " + json.dumps(res), flush=True)
        if fatal:
            sys.exit(3)


# ----------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def child():
    if not os.path.exists(DIAG_LIB):
        pytest.skip("libldmae_hip_diag.so is not built (make -C ldmae_amd/csrc diag)")
    env = dict(os.environ, LDMAE_HIP_LIB=DIAG_LIB)
    env.pop("LDMAE_TUNE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
    results = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            d = json.loads(ln[7:])
            results[d["name"]] = d
    print("\nworst |got - ref| / bound per case (default | variant):")
    for d in results.values():
        print(f"  {d['name']:34s} {d.get('default', '')} | {d.get('variant', '')}")
    return results, r


def test_case_names_are_unique():
    names = [c["name"] for c in CASES]
    assert len(names) == len(set(names)) and 11 not in [k for c in CASES for k, _ in c["keys"]]


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_diag_gemm_case(child, name):
    results, r = child
    assert name in results, f"the child (exit {r.returncode}) ended before this case:\n{r.stderr[-3000:]}"
    assert results[name]["ok"], results[name]["msg"]


def test_child_ran_to_the_end(child):
    results, r = child
    assert r.returncode == 0 and len(results) == len(CASES), r.stderr[-3000:]


if __name__ == "__main__":
    if "--child" in sys.argv:
        _child()
