"""The attention knobs of the diagnostic library (the prefetch-depth keys of csrc/attention.hip), element by element, with the bounds of
tests/attn_check.py.

The product library holds none of this code, so the module starts ONE child Python process with LDMAE_HIP_LIB pointing at
libldmae_hip_diag.so; the child runs every case of CASES and prints one result line per case, the tests below each look one up.  Every
case runs the default path (all tune keys 0 = the shipped behaviour) and then the variant on fresh NaN-filled, canary-guarded buffers
(Guard of test_gpu_attention_paths.py); both are checked per element against the f64 reference with the PRODUCT path's bound.  o and lse
come from the f64 reference, as in test_gpu_attention_paths.py.  Every key is reset to 0 between cases.

  prefetch depth (keys 23 = fused dK/dV, 24 = fused dQ, 25 = the plain pair; 1 / 2 = that depth, 3 = none) on one head-dim-64 fused case and
      one head-dim-16 plain case: the same arithmetic in the same order, so every output is BITWISE equal to the shipped depth's.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "ldmae_amd", "libldmae_hip_diag.so")


def _case_table():
    cs = []
    for key in (23, 24, 25):
        for val in (1, 2, 3):
            cs.append(dict(name=f"prefetch_qkn64_key{key}_{val}", kind="qkn", mode="norm", B=1, H=2, N=192, hd=64, key=key, val=val, bitwise=True))
            cs.append(dict(name=f"prefetch_plain16_key{key}_{val}", kind="plain", dtype="bf16", B=1, H=3, N=256, hd=16, key=key, val=val, bitwise=True))
    return cs


CASES = _case_table()
KEYS = (23, 24, 25)


# ----------------------------------------------------------------------------- the child process
def _child():
    from types import SimpleNamespace

    import torch

    sys.path.insert(0, ROOT)
    import attn_check as ac
    import gemm_check as gc
    from test_gpu_attention_paths import BF16, F16, F32, Guard, _bits, _dt, _stream, _tok
    from ldmae_amd import _lib

    lib = _lib.load()
    assert lib.ldmae_arch() == b"gfx950" and hasattr(lib, "ldmae_tune"), "the child needs the diagnostic library"
    setups, defaults = {}, {}

    def setup(c):
        """Inputs, reference and bounds of a shape: made once, shared by its cases, never modified."""
        dtype = {"bf16": BF16, "fp16": F16}[c.get("dtype", "bf16")]
        key = (c["kind"], c.get("mode"), dtype, c["B"], c["H"], c["N"], c["hd"])
        if key in setups:
            return key, setups[key]
        B, H, N, hd = c["B"], c["H"], c["N"], c["hd"]
        scale = float(hd ** -0.5)
        q, k, v, do = ac.make_inputs(B, H, N, hd, dtype, "unit", 4100 + N + hd, device="cuda")
        f = ac.fwd_ref(q, k, v, hd ** -0.5)
        assert f["finite"]
        o_in, lse_in = f["o"].to(dtype), f["lse"].float().contiguous()
        S = SimpleNamespace(B=B, H=H, N=N, hd=hd, dtype=dtype, scale=scale, b=ac.bwd_ref(q, k, v, o_in, do, lse_in, scale),
                            o=Guard((B, N, H * hd), dtype, _tok(o_in)), lse=Guard((B, H, N), F32, lse_in), do=Guard((B, N, H * hd), dtype, _tok(do)),
                            qkv=Guard((B, N, 3, H, hd), dtype))
        S.qkv.t[:, :, 2] = v.permute(0, 2, 1, 3)
        if c["kind"] == "plain":
            S.qkv.t[:, :, 0], S.qkv.t[:, :, 1] = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3)
            S.ins = [S.o, S.lse, S.do, S.qkv]
        else:                                            # q / k head-major (post-norm), the packed qkv holds the PRE-norm rows in its q | k slots
            g = torch.Generator().manual_seed(99 + N)
            S.x = torch.randn(2, B, H, N, hd, generator=g).to(dtype).cuda()
            S.qkv.t[:, :, 0], S.qkv.t[:, :, 1] = S.x[0].permute(0, 2, 1, 3), S.x[1].permute(0, 2, 1, 3)
            ang = torch.rand(N, hd // 2, generator=g) * 6.28
            S.cos, S.sin = Guard((N, hd), F32, ang.cos().repeat_interleave(2, 1).cuda()), Guard((N, hd), F32, ang.sin().repeat_interleave(2, 1).cuda())
            S.w = Guard((2, hd), F32, (1 + 0.2 * torch.randn(2, hd, generator=g)).cuda()) if c["mode"] == "norm" else None
            S.q, S.k = Guard(q.shape, dtype, q), Guard(k.shape, dtype, k)
            S.ins = [S.o, S.lse, S.do, S.qkv, S.q, S.k, S.cos, S.sin] + ([S.w] if S.w else [])
        setups[key] = S
        return key, S

    def run_plain(S):
        """ldmae_attention_bwd_qkv -> {dqkv}; the delta workspace has exactly the documented size"""
        B, H, N, hd = S.B, S.H, S.N, S.hd
        delta, dqkv = Guard((2, B, H, (N + 63) // 64 * 64), F32), Guard((B, N, 3, H, hd), S.dtype)
        _lib.call("ldmae_attention_bwd_qkv", _dt(S.dtype), S.qkv.ptr(), S.o.ptr(), S.do.ptr(), S.lse.ptr(), dqkv.ptr(), delta.ptr(), B, H, N, hd, S.scale, _stream())
        torch.cuda.synchronize()
        assert delta.intact() and dqkv.intact() and all(g.intact() for g in S.ins), "a canary around a backward output, the delta workspace or an input changed"
        return {"dqkv": dqkv.t.clone()}

    def check_plain(name, S, out):
        r = {}
        for i, n in enumerate(("dq", "dk", "dv")):
            r[n] = ac.check(f"{name} {n}", out["dqkv"][:, :, i].permute(0, 2, 1, 3), S.b[n], S.b["b" + n])
        return r

    def run_qkn(S):
        """ldmae_attention_bwd_pv_qknorm -> {dqkv, dbias, dw}; the workspace has exactly the size the library reports"""
        B, H, N, hd = S.B, S.H, S.N, S.hd
        nws = lib.ldmae_attention_bwd_pv_qknorm_workspace_bytes(B, H, N, hd)
        assert nws % 4 == 0
        ws, dqkv, db = Guard((nws // 4,), F32), Guard((B, N, 3, H, hd), S.dtype), Guard((3 * H * hd,), F32)
        dw = Guard((2, hd), F32) if S.w else None
        _lib.call("ldmae_attention_bwd_pv_qknorm", _dt(S.dtype), S.q.ptr(), S.k.ptr(), S.qkv.ptr(), S.o.ptr(), S.do.ptr(), S.lse.ptr(),
                  S.w.ptr() if S.w else None, S.w.ptr() + 4 * hd if S.w else None, S.cos.ptr(), S.sin.ptr(), 1e-6, dqkv.ptr(),
                  dw.ptr() if dw else None, dw.ptr() + 4 * hd if dw else None, db.ptr(), ws.ptr(), B, H, N, hd, S.scale, _stream())
        torch.cuda.synchronize()
        assert ws.intact() and dqkv.intact() and db.intact() and (dw is None or dw.intact()) and all(g.intact() for g in S.ins), \
            "a canary around a fused-backward output, its workspace or an input changed"
        out = {"dqkv": dqkv.t.clone(), "dbias": db.t.clone()}
        if dw:
            out["dw"] = dw.t.reshape(-1).clone()
        return out

    def check_qkn(name, S, out):
        """As _run_qkn of test_gpu_attention_paths.py; the v slot by its own bound."""
        B, H, N, hd, b, eps = S.B, S.H, S.N, S.hd, S.b, 1e-6
        dqkv, r, S_w = out["dqkv"], {}, []
        for i, n in enumerate(("dq", "dk")):
            wi = S.w.t[i] if S.w else None
            ref, bound = ac.qknorm_bwd_bound(b[n], b["b" + n], S.x[i], wi, S.cos.t, S.sin.t, eps)
            r[n] = ac.check(f"{name} {n} slot", dqkv[:, :, i].permute(0, 2, 1, 3), ref, bound)
            if S.w:
                _, tn = ac.qknorm_bwd_op(b[n], S.x[i], wi, S.cos.t, S.sin.t, eps)
                _, tb = ac.qknorm_bwd_op(b["b" + n], S.x[i], wi, S.cos.t, S.sin.t, eps, absolute=True)
                _, ta = ac.qknorm_bwd_op(b[n].abs() + b["b" + n], S.x[i], wi, S.cos.t, S.sin.t, eps, absolute=True)
                S_w.append((tn.sum((0, 1, 2)), tb.sum((0, 1, 2)), ta.sum((0, 1, 2))))
        r["dv"] = ac.check(f"{name} dv slot", dqkv[:, :, 2].permute(0, 2, 1, 3), b["dv"], b["bdv"])
        if S.w:
            ref = torch.cat([s[0] for s in S_w])
            fn = torch.cat([s[1] for s in S_w]) + gc.acc_bound(torch.cat([s[2] for s in S_w]), B * H * N + hd)
            r["dw"] = ac.check(f"{name} dwq|dwk", out["dw"], ref, fn + 0.5 * gc.ulp(ref.abs() + fn, F32))
        ref, Sm = gc.colsum_ref(dqkv.reshape(B * N, 3 * H * hd))
        r["dbias"] = gc.check_sum(f"{name} dbias", out["dbias"], ref, Sm, B * N, F32)
        return r

    def same_bits(a, b):
        return all(torch.equal(_bits(a[n]), _bits(b[n])) for n in a)

    fatal = None
    for c in CASES:
        run, check = (run_plain, check_plain) if c["kind"] == "plain" else (run_qkn, check_qkn)
        res = {"name": c["name"], "ok": True, "msg": ""}
        try:
            skey, S = setup(c)
            if skey not in defaults:                                    # the shipped behaviour of the diagnostic build, checked once per shape
                assert all(lib.ldmae_tune_query(k) == 0 for k in KEYS)
                defaults[skey] = run(S)
                res["default"] = check(c["name"] + " (default)", S, defaults[skey])
            assert lib.ldmae_tune(c["key"], c["val"]) == 0, f"{c['name']}: {_lib.last_error()}"
            out = run(S)
            res["variant"] = check(c["name"], S, out)
            if c["bitwise"]:
                assert same_bits(out, defaults[skey]), f"{c['name']}: not bitwise equal to the shipped depth"
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
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_diag_attention_case(child, name):
    results, r = child
    assert name in results, f"the child (exit {r.returncode}) ended before this case:\n{r.stderr[-3000:]}"
    assert results[name]["ok"], results[name]["msg"]


def test_child_ran_to_the_end(child):
    results, r = child
    assert r.returncode == 0 and len(results) == len(CASES), r.stderr[-3000:]


if __name__ == "__main__":
    if "--child" in sys.argv:
        _child()
