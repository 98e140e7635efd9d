"""Every dispatch path of the attention family, element by element, with the bounds of tests/attn_check.py.

A seeded table of cases drives the C ABI directly, so each case controls pointers and layouts.  Each case
  - places q, k, v / qkv, o, dO, lse in NaN-padded buffers and every output (o, lse, dq, dk, dv / dqkv, dwq, dwk, dbias) inside a buffer
    pre-filled with the NaN payload of its type: an unwritten row, a write past N or past the head dim, a write into a slot the entry point
    does not own, and a read past the inputs all fail; the delta and fused-backward workspaces have exactly the documented size and a
    canary tail;
  - checks every element of every output against the f64 reference with the per-element bound, and every canary bit;
  - runs a second time on fresh output buffers and requires bitwise-equal results;
  - asserts the launch-count family;
  - records the worst err / bound per path and output (printed at module teardown).
The backward is fed o and lse made by the f64 reference (rounded to their storage types), never the forward kernel's output.

Dispatch predicates (csrc/attention.hip), each taken and not taken by some case (test_case_table_covers_every_predicate):
  attention_fwd_core / attention_bwd_core: dtype (fp16 -> <16, R, true>; bf16 -> attn_hd_dispatch; f32 -> hd == 16 ? hd16 kernel : attn_hd_dispatch_f32);
  RAGGED = N % 64 != 0 (its own instantiation; the backward then runs prefetch depth 0, whole tiles attn_pf(hd): 1 at head dim 64);
  layouts: head-major (sb, sh, ld) = (H N hd, N hd, hd), packed (N 3 H hd, hd, 3 H hd), mixed (q / k head-major, v packed);
  static shift: SB != NULL && bq <= 50 for every lane of the wave; sb_heads ? (SB[2 bh] > 0 ? sqrt(SB0 SB1) c 1.02 : own norm) : *SB;
  active = q0 < N per wave; xcd_remap: r = grid & 7 (x < r branch) and q = grid >> 3 (0 below 8 workgroups).

First device run (MI355X): every case inside its bound with zero excluded elements, every rerun bitwise equal, no canary touched; the
module takes about 2 s.  Worst err / bound: bf16 / fp16 outputs 0.3 .. 0.94, lse 0.01 .. 0.03 where l sums the unrounded p and 0.2 .. 0.77
at head dims 16 / 72, f32 outputs 0.004 .. 0.05 (the hd + 5 worst-case chain of step 2 of attn_check.py dominates there).
"""
import math

import pytest
import torch

import attn_check as ac
import gemm_check as gc

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
_BITS = {F32: (torch.int32, 0x7FC0DEAD), BF16: (torch.int16, 0x7FDE), F16: (torch.int16, 0x7E5A)}
RATIOS: dict = {}
SEEN: dict = {}


@pytest.fixture(scope="module")
def lib():
    from ldmae_amd import _lib
    assert _lib.load().ldmae_arch() == b"gfx950"
    yield _lib
    if RATIOS:
        print("\nworst |got - ref| / bound per path and output:")
        for k in sorted(RATIOS):
            print(f"  {k:44s} {RATIOS[k]:.3f}")


def _dt(dtype):
    return {F32: 0, BF16: 1, F16: 2}[dtype]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


def _note(name, v):
    SEEN.setdefault(name, set()).add(bool(v))


class Guard:
    """A contiguous tensor of `shape` inside a flat buffer whose every other element (128 in front, 2048 behind) holds the NaN payload."""

    def __init__(self, shape, dtype, init=None, front=128, back=2048):
        it, bits = _BITS[dtype]
        n = math.prod(shape)
        self.it, self.bits, self.n, self.front = it, bits, n, front
        self.buf = torch.empty(front + n + back, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.buf.view(it).fill_(bits)
        self.t = self.buf[front:front + n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        b = self.buf.view(self.it)
        return bool((b[:self.front] == self.bits).all() and (b[self.front + self.n:] == self.bits).all())

    def untouched(self, view):
        return bool((view.view(self.it) == self.bits).all())

    def ptr(self):
        return self.t.data_ptr()


def _bits(t):
    return t.contiguous().view(_BITS[t.dtype][0])


def _hm(tok, B, H, N, hd):
    """token-major [B,N,H*hd] -> head-major [B,H,N,hd]"""
    return tok.view(B, N, H, hd).permute(0, 2, 1, 3)


def _tok(hm):
    B, H, N, hd = hm.shape
    return hm.permute(0, 2, 1, 3).reshape(B, N, H * hd)


# ----------------------------------------------------------------------------- the table
def C(name, dtype, hd, B, H, N, layout="hm", fam="unit", bound=None, bwd=True, gain=None, qkn=None):
    return dict(name=name, dtype=dtype, hd=hd, B=B, H=H, N=N, layout=layout, fam=fam, bound=bound, bwd=bwd, gain=gain, qkn=qkn)


CASES = [
    # bf16 / fp16 flash kernels.  grid = B H ceil(N / 128) is noted behind each case (xcd_remap: below 8, multiple of 8, 8 q + r)
    C("bf16_64_dit256_pv_bound_low", BF16, 64, 1, 12, 256, "pv", bound=("scalar", "low")),                 # 24
    C("bf16_64_dit1024_pv_peaked_49", BF16, 64, 1, 12, 1024, "pv", "peaked", bound=("scalar", 49.5)),      # 96
    C("bf16_64_pv_peaked_51_tracked", BF16, 64, 1, 3, 256, "pv", "peaked", bound=("scalar", 50.5), bwd=False),   # 6
    C("bf16_16_vmae256_qkv_ownnorm", BF16, 16, 1, 12, 256, "qkv", bound=("heads", "own")),                # 24
    C("bf16_16_vmae1024_qkv_qmax", BF16, 16, 1, 12, 1024, "qkv", bound=("heads", "qmax")),                # 96
    C("bf16_16_qkv_heads_all_above", BF16, 16, 1, 3, 200, "qkv", gain=[2.6, 2.6, 2.6], bound=("heads", "qmax"), bwd=False),   # 6
    C("bf16_16_qkv_heads_mixed", BF16, 16, 2, 3, 200, "qkv", gain=[1.0, 2.6, 1.0], bound=("heads", "qmax"), bwd=False),       # 12
    C("bf16_16_qkv_ownnorm_mixed_ragged", BF16, 16, 1, 5, 257, "qkv", gain=[1.0, 1.9, 1.0, 2.6, 1.0], bound=("heads", "own"), bwd=False),   # 15
    C("bf16_16_qkv_ragged_peaked", BF16, 16, 2, 3, 200, "qkv", "peaked"),                                 # 12
    C("bf16_16_qkv_N1", BF16, 16, 1, 1, 1, "qkv"),                                                         # 1
    C("bf16_32_hm_128", BF16, 32, 1, 3, 128),                                                              # 3
    C("bf16_32_hm_ragged257", BF16, 32, 1, 5, 257, fam="peaked"),                                          # 15
    C("bf16_64_pv_ragged200", BF16, 64, 1, 3, 200, "pv"),                                                  # 6
    C("bf16_64_hm_N40", BF16, 64, 1, 9, 40),                                                               # 9
    C("bf16_64_hm_N20", BF16, 64, 1, 10, 20, fam="peaked"),                                                # 10
    C("bf16_64_hm_N64", BF16, 64, 1, 13, 64),                                                              # 13
    C("bf16_64_qkv_N224", BF16, 64, 1, 7, 224, "qkv"),                                                     # 14
    C("bf16_64_hm_N448_peaked", BF16, 64, 1, 2, 448, fam="peaked"),                                        # 8, seven tiles: more than two wraps of the ring
    C("bf16_72_hm_256", BF16, 72, 2, 5, 256, fam="peaked"),                                                # 20
    C("bf16_72_hm_ragged100", BF16, 72, 1, 11, 100),                                                       # 11
    C("bf16_72_pv_ragged130", BF16, 72, 1, 2, 130, "pv"),                                                  # 4
    C("bf16_128_hm_128", BF16, 128, 1, 2, 128),                                                            # 2
    C("bf16_128_pv_ragged130", BF16, 128, 1, 13, 130, "pv", "peaked"),                                     # 26
    C("fp16_16_qkv_256", F16, 16, 1, 12, 256, "qkv"),                                                      # 24
    C("fp16_16_hm_ragged200_peaked", F16, 16, 2, 3, 200, fam="peaked"),                                    # 12
    C("fp16_16_hm_N20", F16, 16, 1, 1, 20),                                                                # 1
    # fused backward (QK-norm / RoPE adjoint in the epilogues)
    C("bf16_64_qkn_norm_128", BF16, 64, 2, 3, 128, "pv", qkn="norm"),
    C("bf16_64_qkn_norm_dit256", BF16, 64, 1, 12, 256, "pv", qkn="norm_split"),
    C("bf16_64_qkn_rope_192", BF16, 64, 1, 2, 192, "pv", "peaked", qkn="rope"),
    C("bf16_128_qkn_norm_192", BF16, 128, 1, 2, 192, "pv", qkn="norm"),
    C("bf16_128_qkn_rope_64", BF16, 128, 1, 3, 64, "pv", qkn="rope"),
    # f32 kernels
    C("f32_16_hm_ragged200", F32, 16, 2, 3, 200, fam="peaked"),
    C("f32_16_qkv_256", F32, 16, 1, 12, 256, "qkv", bwd=False),
    C("f32_16_hm_N1", F32, 16, 1, 1, 1),
    C("f32_16_hm_128", F32, 16, 1, 2, 128),
    C("f32_32_hm_128", F32, 32, 1, 3, 128),
    C("f32_32_hm_ragged40", F32, 32, 1, 2, 40, fam="peaked"),
    C("f32_64_hm_256", F32, 64, 1, 3, 256, fam="peaked"),
    C("f32_64_hm_ragged257", F32, 64, 1, 2, 257),
    C("f32_72_hm_ragged100", F32, 72, 1, 2, 100),
    C("f32_72_hm_128", F32, 72, 1, 2, 128, fam="peaked"),
    C("f32_80_hm_ragged200", F32, 80, 1, 2, 200),
    C("f32_80_hm_64", F32, 80, 1, 1, 64),
    C("f32_96_hm_192", F32, 96, 1, 2, 192),
    C("f32_96_hm_ragged130", F32, 96, 1, 1, 130, fam="peaked"),
    C("f32_128_hm_128_fwd", F32, 128, 1, 2, 128, bwd=False),
    C("f32_128_hm_ragged100_fwd", F32, 128, 1, 2, 100, fam="peaked", bwd=False),
]


def test_case_names_are_unique():
    names = [c["name"] for c in CASES]
    assert len(names) == len(set(names))


# ----------------------------------------------------------------------------- one case
def _inputs(c):
    B, H, N, hd, dtype = c["B"], c["H"], c["N"], c["hd"], c["dtype"]
    q, k, v, do = ac.make_inputs(B, H, N, hd, dtype, c["fam"], 7000 + sum(map(ord, c["name"])), device="cuda", gain=c["gain"])
    G = {}
    if c["layout"] == "hm":
        G["q"], G["k"], G["v"] = Guard(q.shape, dtype, q), Guard(k.shape, dtype, k), Guard(v.shape, dtype, v)
    else:
        G["qkv"] = Guard((B, N, 3, H, hd), dtype)                       # q | k slots stay NaN in the mixed layout: they must not be read
        G["qkv"].t[:, :, 2] = v.permute(0, 2, 1, 3)
        if c["layout"] == "qkv":
            G["qkv"].t[:, :, 0], G["qkv"].t[:, :, 1] = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3)
        else:
            G["q"], G["k"] = Guard(q.shape, dtype, q), Guard(k.shape, dtype, k)
    G["do"] = Guard((B, N, H * hd), dtype, _tok(do))
    return q, k, v, do, G


def _fwd_call(lib, c, G, entry, o, lse, sb=None):
    B, H, N, hd, d = c["B"], c["H"], c["N"], c["hd"], _dt(c["dtype"])
    s, st = float(hd ** -0.5), _stream()
    if entry == "fwd":
        lib.call("ldmae_attention_fwd", d, G["q"].ptr(), G["k"].ptr(), G["v"].ptr(), o.ptr(), lse.ptr(), B, H, N, hd, s, st)
    elif entry == "fwd_qkv":
        lib.call("ldmae_attention_fwd_qkv", d, G["qkv"].ptr(), o.ptr(), lse.ptr(), B, H, N, hd, s, st)
    elif entry == "fwd_qkv_bounded":
        lib.call("ldmae_attention_fwd_qkv_bounded", d, G["qkv"].ptr(), o.ptr(), lse.ptr(), sb.data_ptr(), B, H, N, hd, s, st)
    elif entry == "fwd_pv":
        lib.call("ldmae_attention_fwd_pv", d, G["q"].ptr(), G["k"].ptr(), G["qkv"].ptr(), o.ptr(), lse.ptr(), B, H, N, hd, s, st)
    elif entry == "fwd_pv_bounded":
        lib.call("ldmae_attention_fwd_pv_bounded", d, G["q"].ptr(), G["k"].ptr(), G["qkv"].ptr(), o.ptr(), lse.ptr(), sb.data_ptr(), B, H, N, hd, s, st)
    else:
        raise AssertionError(entry)


def _fam(dtype):
    return {F32: "attn_f32", BF16: "attn_bf16", F16: "attn_f16"}[dtype]


def _counts_ok(counts, dtype, n=1):
    assert counts[_fam(dtype)] == n and all(v == 0 for k, v in counts.items() if k.startswith("attn") and k != _fam(dtype)), counts


def _run_fwd(lib, c, G, entry, sb=None):
    B, H, N, hd, dtype = c["B"], c["H"], c["N"], c["hd"], c["dtype"]
    res = []
    for _ in range(2):
        o, lse = Guard((B, N, H * hd), dtype), Guard((B, H, N), F32)
        lib.launch_counts(reset=True)
        _fwd_call(lib, c, G, entry, o, lse, sb)
        counts = lib.launch_counts()
        torch.cuda.synchronize()
        _counts_ok(counts, dtype)
        assert o.intact() and lse.intact(), f"{entry}: a canary around o / lse changed"
        res.append((o.t.clone(), lse.t.clone()))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1])), f"{entry}: rerun not bitwise equal"
    return res[0]


def _shift_for(lib, c, q, k, G, f):
    """-> (entry, SB tensor, shift [B,H,N] of the bound the kernel derives, heads whose every bound is above 50)."""
    B, H, N, hd = c["B"], c["H"], c["N"], c["hd"]
    kind, val = c["bound"]
    c32 = ac.c32(hd ** -0.5)
    if kind == "scalar":
        smax = float(f["smax"].max())
        val = math.ceil(smax * 1.05) if val == "low" else val
        assert smax <= val, f"the bound {val} is not a bound of the reference scores ({smax})"
        _note("scalar bound <= 50", val <= 50)
        _note("scalar bound well below 50", val < 25)
        sb = torch.full((1,), float(val), device="cuda")
        return "fwd_pv_bounded", sb, torch.full((B, H, N), float(val), device="cuda"), (list(range(B * H)) if val > 50 else [])
    k2 = (k.float() ** 2).sum(-1).amax(-1).reshape(-1)
    if val == "own":
        sb = torch.empty(B * H, 2, device="cuda")
        lib.call("ldmae_k_norm_max", G["qkv"].ptr(), sb.data_ptr(), B, N, H, hd, _stream())
        assert torch.equal(sb[:, 0], torch.zeros(B * H, device="cuda"))
        assert bool((sb[:, 1].double() >= k2.double() * (1 - 1e-6)).all()) and bool((sb[:, 1].double() <= k2.double() * (1 + 1e-5)).all())
        qs = ac.scaled(q, hd ** -0.5, "mfma16").float()
        shift = torch.sqrt((qs * qs).sum(-1) * sb[:, 1].view(B, H, 1)) * 1.02 + 0.01
    else:
        q2 = (q.float() ** 2).sum(-1).amax(-1).reshape(-1) * (1 + 1e-6)
        sb = torch.stack([q2, k2 * (1 + 1e-6)], 1).contiguous()
        shift = (torch.sqrt(sb[:, 0] * sb[:, 1]) * c32 * 1.02).view(B, H, 1).expand(B, H, N).contiguous()
    assert bool((shift.double() >= f["smax"]).all()), "the derived bound is not a bound of the reference scores"
    _note("per-head query maximum > 0", val == "qmax")
    above = (shift > 50).reshape(B * H, N)
    cls = "all above" if bool(above.all()) else ("all below" if not bool(above.any()) else "mixed")
    for name in ("all above", "all below", "mixed"):
        _note(f"per-head bounds: {name}", cls == name)
    return "fwd_qkv_bounded", sb, shift, [i for i in range(B * H) if bool(above[i].all())]


def _check_fwd(c, tag, f, o, lse):
    B, H, N, hd = c["B"], c["H"], c["N"], c["hd"]
    path = f"{ac.kind_of(c['dtype'], hd)}[{str(c['dtype'])[6:]},{hd}{',ragged' if N % 64 else ''}]/{tag}"
    _record(path + ":o", ac.check(c["name"] + " o", _hm(o, B, H, N, hd), f["o"], f["bo"]))
    _record(path + ":lse", ac.check(c["name"] + " lse", lse, f["lse"], f["bl"]))


def _run_bwd(lib, c, q, k, v, do, G, f):
    B, H, N, hd, dtype = c["B"], c["H"], c["N"], c["hd"], c["dtype"]
    scale, d, st = float(hd ** -0.5), _dt(dtype), _stream()
    o_in, lse_in = f["o"].to(dtype), f["lse"].float().contiguous()
    Go, Gl = Guard((B, N, H * hd), dtype, _tok(o_in)), Guard((B, H, N), F32, lse_in)
    b = ac.bwd_ref(q, k, v, o_in, do, lse_in, scale)
    NP = (N + 63) // 64 * 64
    lay = c["layout"]
    res = []
    for _ in range(2):
        delta = Guard((2, B, H, NP), F32)                  # exactly the documented [2][B,H,NP]
        out = {}
        lib.launch_counts(reset=True)
        if lay == "hm":
            out = {n: Guard((B, H, N, hd), dtype) for n in ("dq", "dk", "dv")}
            lib.call("ldmae_attention_bwd", d, G["q"].ptr(), G["k"].ptr(), G["v"].ptr(), Go.ptr(), G["do"].ptr(), Gl.ptr(), out["dq"].ptr(),
                     out["dk"].ptr(), out["dv"].ptr(), delta.ptr(), B, H, N, hd, scale, st)
        elif lay == "qkv":
            out = {"dqkv": Guard((B, N, 3, H, hd), dtype)}
            lib.call("ldmae_attention_bwd_qkv", d, G["qkv"].ptr(), Go.ptr(), G["do"].ptr(), Gl.ptr(), out["dqkv"].ptr(), delta.ptr(), B, H, N, hd, scale, st)
        else:
            out = {"dq": Guard((B, H, N, hd), dtype), "dk": Guard((B, H, N, hd), dtype), "dqkv": Guard((B, N, 3, H, hd), dtype)}
            lib.call("ldmae_attention_bwd_pv", d, G["q"].ptr(), G["k"].ptr(), G["qkv"].ptr(), Go.ptr(), G["do"].ptr(), Gl.ptr(), out["dq"].ptr(),
                     out["dk"].ptr(), out["dqkv"].ptr(), delta.ptr(), B, H, N, hd, scale, st)
        counts = lib.launch_counts()
        torch.cuda.synchronize()
        _counts_ok(counts, dtype)
        assert delta.intact() and all(g.intact() for g in out.values()), "a canary around a backward output or the delta workspace changed"
        if lay == "pv":
            assert out["dqkv"].untouched(out["dqkv"].t[:, :, :2]), "attention_bwd_pv wrote into the q | k slots of dqkv"
        res.append({n: g.t.clone() for n, g in out.items()})
    for n in res[0]:
        assert torch.equal(_bits(res[0][n]), _bits(res[1][n])), f"backward {n}: rerun not bitwise equal"
    r = res[0]
    if lay == "hm":
        got = (r["dq"], r["dk"], r["dv"])
    elif lay == "qkv":
        got = tuple(r["dqkv"][:, :, i].permute(0, 2, 1, 3) for i in range(3))
    else:
        got = (r["dq"], r["dk"], r["dqkv"][:, :, 2].permute(0, 2, 1, 3))
    path = f"{ac.kind_of(dtype, hd)}[{str(dtype)[6:]},{hd}{',ragged' if N % 64 else ''}]/bwd_{lay}"
    for n, g in zip(("dq", "dk", "dv"), got):
        _record(f"{path}:{n}", ac.check(f"{c['name']} {n}", g, b[n], b["b" + n]))
    return b, got, Go, Gl


def _run_qkn(lib, c, q, k, v, do, G, f):
    """ldmae_attention_bwd_pv_qknorm: dv slot bit for bit attention_bwd_pv's; q | k slots, dwq, dwk, dbias by bound."""
    B, H, N, hd, dtype = c["B"], c["H"], c["N"], c["hd"], c["dtype"]
    scale, st, eps = float(hd ** -0.5), _stream(), 1e-6
    b, got, Go, Gl = _run_bwd(lib, c, q, k, v, do, G, f)
    g = torch.Generator().manual_seed(99 + N)
    x = torch.randn(2, B, H, N, hd, generator=g).to(dtype).cuda()                     # pre-norm q | k rows of the packed qkv
    G["qkv"].t[:, :, 0], G["qkv"].t[:, :, 1] = x[0].permute(0, 2, 1, 3), x[1].permute(0, 2, 1, 3)
    ang = torch.rand(N, hd // 2, generator=g) * 6.28
    cos, sin = Guard((N, hd), F32, ang.cos().repeat_interleave(2, 1).cuda()), Guard((N, hd), F32, ang.sin().repeat_interleave(2, 1).cuda())
    norm = c["qkn"] != "rope"
    w = Guard((2, hd), F32, (1 + 0.2 * torch.randn(2, hd, generator=g)).cuda()) if norm else None
    nws = lib.load().ldmae_attention_bwd_pv_qknorm_workspace_bytes(B, H, N, hd)
    assert nws % 4 == 0
    res = []
    for _ in range(2):
        ws = Guard((nws // 4,), F32)
        dqkv, db = Guard((B, N, 3, H, hd), dtype), Guard((3 * H * hd,), F32)
        if c["qkn"] == "norm_split":                            # dwq and dwk NOT adjacent: the library reduces into the workspace and copies
            dwq, dwk = Guard((hd,), F32), Guard((hd,), F32)
            pq, pk = dwq.ptr(), dwk.ptr()
        elif norm:
            dwq = dwk = Guard((2, hd), F32)
            pq, pk = dwq.ptr(), dwq.ptr() + 4 * hd
        else:
            dwq = dwk = None
            pq = pk = None
        lib.launch_counts(reset=True)
        lib.call("ldmae_attention_bwd_pv_qknorm", _dt(dtype), G["q"].ptr(), G["k"].ptr(), G["qkv"].ptr(), Go.ptr(), G["do"].ptr(), Gl.ptr(),
                 w.ptr() if norm else None, w.ptr() + 4 * hd if norm else None, cos.ptr(), sin.ptr(), eps, dqkv.ptr(), pq, pk, db.ptr(), ws.ptr(),
                 B, H, N, hd, scale, st)
        counts = lib.launch_counts()
        torch.cuda.synchronize()
        _counts_ok(counts, dtype)
        assert ws.intact() and dqkv.intact() and db.intact() and (not norm or (dwq.intact() and dwk.intact())), "a canary around a fused-backward output changed"
        dw = None if not norm else (torch.cat([dwq.t, dwk.t]) if c["qkn"] == "norm_split" else dwq.t.reshape(-1)).clone()
        res.append((dqkv.t.clone(), db.t.clone(), dw))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(res[0][1], res[1][1]), "fused backward: rerun not bitwise equal"
    dqkv, db, dw = res[0]
    assert torch.equal(_bits(dqkv[:, :, 2].permute(0, 2, 1, 3)), _bits(got[2])), "dv slot differs from attention_bwd_pv"
    path = f"qknorm[{hd},{c['qkn'].split('_')[0]}]"
    S_w = []
    for i, n in enumerate(("dq", "dk")):
        wi = w.t[i] if norm else None
        ref, bound = ac.qknorm_bwd_bound(b[n], b["b" + n], x[i], wi, cos.t, sin.t, eps)
        _record(f"{path}:{n}-slot", ac.check(f"{c['name']} {n} slot", dqkv[:, :, i].permute(0, 2, 1, 3), ref, bound))
        if norm:
            _, tn = ac.qknorm_bwd_op(b[n], x[i], wi, cos.t, sin.t, eps)
            _, tb = ac.qknorm_bwd_op(b["b" + n], x[i], wi, cos.t, sin.t, eps, absolute=True)
            _, ta = ac.qknorm_bwd_op(b[n].abs() + b["b" + n], x[i], wi, cos.t, sin.t, eps, absolute=True)
            S_w.append((tn.sum((0, 1, 2)), tb.sum((0, 1, 2)), ta.sum((0, 1, 2))))
    if norm:
        ref = torch.cat([s[0] for s in S_w])
        push, S = torch.cat([s[1] for s in S_w]), torch.cat([s[2] for s in S_w])
        fn = push + gc.acc_bound(S, B * H * N + hd)                # fixed-order f32 sums over the rows; t n itself: a few roundings, inside the hd
        _record(f"{path}:dw", ac.check(f"{c['name']} dwq|dwk", dw, ref, fn + 0.5 * gc.ulp(ref.abs() + fn, F32)))
    stored = dqkv.reshape(B * N, 3 * H * hd)
    ref, S = gc.colsum_ref(stored)
    _record(f"{path}:dbias", gc.check_sum(f"{c['name']} dbias", db, ref, S, B * N, F32))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_attention_path(lib, case):
    c = case
    B, H, N, hd, dtype = c["B"], c["H"], c["N"], c["hd"], c["dtype"]
    q, k, v, do, G = _inputs(c)
    f = ac.fwd_ref(q, k, v, hd ** -0.5)
    assert f["finite"]
    if c["fam"] == "peaked" and N >= 40:
        assert float(f["s2"].amax(-1).max()) >= 25
    entry = {"hm": "fwd", "qkv": "fwd_qkv", "pv": "fwd_pv"}[c["layout"]]
    o, lse = _run_fwd(lib, c, G, entry)
    _check_fwd(c, entry, f, o, lse)
    if c["bound"]:
        bentry, sb, shift, tracked_heads = _shift_for(lib, c, q, k, G, f)
        fs = ac.fwd_ref(q, k, v, hd ** -0.5, shift=shift)
        ob, lseb = _run_fwd(lib, c, G, bentry, sb)
        _check_fwd(c, bentry, fs, ob, lseb)
        oh, obh = _hm(o, B, H, N, hd).reshape(B * H, N, hd), _hm(ob, B, H, N, hd).reshape(B * H, N, hd)
        for i in tracked_heads:                                # bound above 50: the tracked form, bit for bit
            assert torch.equal(_bits(oh[i]), _bits(obh[i])) and torch.equal(lse.view(B * H, N)[i], lseb.view(B * H, N)[i]), f"head {i}: not the tracked form"
        if c["bound"][0] == "scalar" and not tracked_heads:
            assert not torch.equal(lse, lseb) or N == 1        # a static shift was really taken (lse = (bound + log2 l) ln 2 rounds differently)
    if c["qkn"]:
        _run_qkn(lib, c, q, k, v, do, G, f)
    elif c["bwd"]:
        _run_bwd(lib, c, q, k, v, do, G, f)
    for g in G.values():
        assert g.intact()


def test_case_table_covers_every_predicate():
    """Every dispatch predicate restated in the module docstring is both taken and not taken by some case.  (The static-shift predicates
    are noted while the cases run: run the whole module.)"""
    seen = {}

    def note(name, v):
        seen.setdefault(name, set()).add(bool(v))

    grids16, ractive = set(), set()
    for c in CASES:
        dtype, hd, N, B, H = c["dtype"], c["hd"], c["N"], c["B"], c["H"]
        fam = str(dtype)[6:]
        for x in (BF16, F16, F32):
            note(f"dtype {str(x)[6:]}", dtype == x)
        note(f"RAGGED fwd [{fam},{hd}]", N % 64 != 0)
        if c["bwd"] or c["qkn"]:
            note(f"RAGGED bwd [{fam},{hd}]", N % 64 != 0)
            note(f"bwd layout {c['layout']} ragged", N % 64 != 0)
        if dtype == BF16 and hd == 64 and (c["bwd"] or c["qkn"]):
            note("backward prefetch depth 1 (hd 64, whole tiles)", N % 64 == 0)
        if dtype == F32:
            note("f32 hd16 kernel", hd == 16)
            if hd == 16:
                note("f32 hd16 packed layout", c["layout"] == "qkv")
        for lay in ("hm", "qkv", "pv"):
            note(f"layout {lay}", c["layout"] == lay)
        note("static bound given", c["bound"] is not None)
        if c["bound"]:
            note("sb_heads", c["bound"][0] == "heads")
        if c["qkn"]:
            note("fused backward with wq / wk", c["qkn"] != "rope")
            note("fused backward dwq | dwk adjacent", c["qkn"] != "norm_split")
            note("fused backward head dim 128", hd == 128)
            note("fused backward N % 128 == 0 (all four waves active)", N % 128 == 0)
        note("fused backward", c["qkn"] is not None)
        note("family peaked", c["fam"] == "peaked")
        note("B == 1", B == 1)
        note("H == 1", H == 1)
        nt = (N + 63) // 64
        note("one tile", nt == 1)
        note("N < 32 (three waves idle)", N < 32)
        note("fewer tiles than ring stages", nt < 3)
        note("more than two wraps of the ring", nt > 6)
        note("N == 64", N == 64)
        note("N == 128", N == 128)
        note("N == 1", N == 1)
        if dtype != F32:
            grid = B * H * ((N + 127) // 128)
            grids16.add((grid < 8, grid % 8))
            ractive.add(min(4, ((N - 1) % 128) // 32 + 1))
    assert {r for small, r in grids16 if not small} == set(range(8)), f"xcd_remap remainders seen on grids >= 8: {sorted(grids16)}"
    assert any(small for small, _ in grids16)
    assert ractive == {1, 2, 3, 4}, f"active waves in the last workgroup: {ractive}"
    heads_bf16 = {c["hd"] for c in CASES if c["dtype"] == BF16}
    assert heads_bf16 == {16, 32, 64, 72, 128}
    assert {c["hd"] for c in CASES if c["dtype"] == F32} == {16, 32, 64, 72, 80, 96, 128}
    assert {c["hd"] for c in CASES if c["dtype"] == F32 and c["bwd"]} == {16, 32, 64, 72, 80, 96}
    for name, vals in seen.items():
        assert vals == {True, False}, f"predicate {name!r} is only ever {vals}"
    if SEEN:
        for name, vals in SEEN.items():
            assert vals == {True, False}, f"predicate {name!r} (noted at run time) is only ever {vals}"
        assert {"scalar bound <= 50", "per-head query maximum > 0", "per-head bounds: mixed", "per-head bounds: all above", "per-head bounds: all below"} <= set(SEEN)


# ----------------------------------------------------------------------------- refusals
def test_refusals_are_loud_and_write_nothing(lib):
    B, H, N = 1, 2, 128
    st = _stream()

    def bufs(dtype, hd, n=N):
        ins = [Guard((B, H, n, hd), dtype, torch.randn(B, H, n, hd, device="cuda").to(dtype)) for _ in range(3)]
        outs = [Guard((B, H, n, hd), dtype) for _ in range(3)]
        o, lse, do = Guard((B, n, H * hd), dtype), Guard((B, H, n), F32), Guard((B, n, H * hd), dtype, torch.randn(B, n, H * hd, device="cuda").to(dtype))
        delta = Guard((2, B, H, (n + 63) // 64 * 64), F32)
        return ins, outs, o, lse, do, delta

    def clean(*gs):
        torch.cuda.synchronize()
        for g in gs:
            assert g.intact() and g.untouched(g.t), "a refused call wrote something"

    ins, outs, o, lse, do, delta = bufs(F32, 128)
    oin, lin = Guard((B, N, H * 128), F32, torch.zeros(B, N, H * 128, device="cuda")), Guard((B, H, N), F32, torch.zeros(B, H, N, device="cuda"))
    with pytest.raises(RuntimeError, match=r"attention_bwd\(f32\): head_dim 128 needs more than the 160 KiB of LDS"):
        lib.call("ldmae_attention_bwd", 0, ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), oin.ptr(), do.ptr(), lin.ptr(), outs[0].ptr(), outs[1].ptr(),
                 outs[2].ptr(), delta.ptr(), B, H, N, 128, 0.1, st)
    clean(*outs, delta)
    ins, outs, o, lse, do, delta = bufs(F16, 32)
    with pytest.raises(RuntimeError, match=r"attention_fwd\(fp16\): head_dim 16 only"):
        lib.call("ldmae_attention_fwd", 2, ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), o.ptr(), lse.ptr(), B, H, N, 32, 0.1, st)
    with pytest.raises(RuntimeError, match=r"attention_bwd\(fp16\): head_dim 16 only"):
        lib.call("ldmae_attention_bwd", 2, ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), o.ptr(), do.ptr(), lse.ptr(), outs[0].ptr(), outs[1].ptr(),
                 outs[2].ptr(), delta.ptr(), B, H, N, 32, 0.1, st)
    clean(o, lse, *outs, delta)
    qkv16 = Guard((B, N, 3, H, 16), F16, torch.randn(B, N, 3, H, 16, device="cuda").to(F16))
    sb = torch.ones(B * H, 2, device="cuda")
    o16, lse16 = Guard((B, N, H * 16), F16), Guard((B, H, N), F32)
    with pytest.raises(RuntimeError, match="attention_fwd_qkv_bounded: bf16 only"):
        lib.call("ldmae_attention_fwd_qkv_bounded", 2, qkv16.ptr(), o16.ptr(), lse16.ptr(), sb.data_ptr(), B, H, N, 16, 0.25, st)
    clean(o16, lse16)
    for hd, n, msg in ((72, 128, r"head_dim 72 \(64 or 128"), (64, 200, r"N=200 must be a multiple of 64")):
        ins, outs, o, lse, do, delta = bufs(BF16, hd, n)
        qkv, dqkv = Guard((B, n, 3, H, hd), BF16, torch.randn(B, n, 3, H, hd, device="cuda").to(BF16)), Guard((B, n, 3, H, hd), BF16)
        tab = torch.ones(n, hd, device="cuda")
        w, dw, db = torch.ones(2, hd, device="cuda"), Guard((2, hd), F32), Guard((3 * H * hd,), F32)
        ws = Guard((1 << 20,), F32)
        with pytest.raises(RuntimeError, match="attention_bwd_pv_qknorm: " + msg):
            lib.call("ldmae_attention_bwd_pv_qknorm", 1, ins[0].ptr(), ins[1].ptr(), qkv.ptr(), o.ptr(), do.ptr(), lse.ptr(), w.data_ptr(),
                     w.data_ptr() + 4 * hd, tab.data_ptr(), tab.data_ptr(), 1e-6, dqkv.ptr(), dw.ptr(), dw.ptr() + 4 * hd, db.ptr(), ws.ptr(), B, H, n,
                     hd, 0.1, st)
        clean(dqkv, dw, db, ws)
    ins, outs, o, lse, do, delta = bufs(BF16, 16)
    with pytest.raises(RuntimeError, match="attention_bwd: head_dim 12 must be a multiple of 8"):
        lib.call("ldmae_attention_bwd", 1, ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), o.ptr(), do.ptr(), lse.ptr(), outs[0].ptr(), outs[1].ptr(),
                 outs[2].ptr(), delta.ptr(), B, H, N, 12, 0.1, st)
    with pytest.raises(RuntimeError, match=r"attention\(bf16\): head_dim 24 unsupported"):
        lib.call("ldmae_attention_fwd", 1, ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), o.ptr(), lse.ptr(), B, H, 64, 24, 0.1, st)
    with pytest.raises(RuntimeError, match="attention_fwd: null pointer"):
        lib.call("ldmae_attention_fwd", 1, ins[0].ptr(), None, ins[2].ptr(), o.ptr(), lse.ptr(), B, H, N, 16, 0.1, st)
    with pytest.raises(RuntimeError, match="attention_bwd: null pointer"):
        lib.call("ldmae_attention_bwd", 1, ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), o.ptr(), do.ptr(), lse.ptr(), outs[0].ptr(), outs[1].ptr(),
                 outs[2].ptr(), None, B, H, N, 16, 0.1, st)
    clean(o, lse, *outs, delta)


# ----------------------------------------------------------------------------- the Python wrappers' padding route
@pytest.fixture(scope="module")
def ops(lib):
    from ldmae_amd import ops
    return ops


@pytest.mark.parametrize("dtype,hd", [(BF16, 8), (BF16, 24), (BF16, 40), (BF16, 80), (F32, 8), (F32, 24)])
def test_wrapper_padding_route(ops, dtype, hd):
    """Head dims outside the instantiated set: ops pads to the next kernel, slices and reshapes.  Same per-element check, through ops; the
    reference and the bound are those of the padded problem (zero columns change neither)."""
    B, H, N = 2, 3, 100
    P = ops._attn_pad(hd, dtype)
    q, k, v, do = ac.make_inputs(B, H, N, hd, dtype, "unit", 500 + hd, device="cuda")
    scale = hd ** -0.5
    pad = lambda t: torch.nn.functional.pad(t, (0, P - hd))      # noqa: E731
    f = ac.fwd_ref(pad(q), pad(k), pad(v), scale)
    o_in, lse_in = f["o"][..., :hd].to(dtype), f["lse"].float().contiguous()
    b = ac.bwd_ref(pad(q), pad(k), pad(v), pad(o_in), pad(do), lse_in, scale)
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * hd).contiguous()
    for tag, (o, lse) in (("hm", ops.attention_fwd(q, k, v, scale)), ("qkv", ops.attention_fwd_qkv(qkv, B, N, H, hd, scale))):
        assert o.shape == (B, N, H * hd)
        _record(f"ops[{str(dtype)[6:]},{hd}->{P}]/fwd:o", ac.check(f"ops fwd {tag} o", _hm(o, B, H, N, hd), f["o"][..., :hd], f["bo"][..., :hd]))
        _record(f"ops[{str(dtype)[6:]},{hd}->{P}]/fwd:lse", ac.check(f"ops fwd {tag} lse", lse, f["lse"], f["bl"]))
    dq, dk, dv = ops.attention_bwd(q, k, v, _tok(o_in).contiguous(), _tok(do).contiguous(), lse_in, scale)
    dqkv = ops.attention_bwd_qkv(qkv, _tok(o_in).contiguous(), _tok(do).contiguous(), lse_in, B, N, H, hd, scale).view(B, N, 3, H, hd)
    for i, (n, g) in enumerate((("dq", dq), ("dk", dk), ("dv", dv))):
        assert g.shape == (B, H, N, hd)
        _record(f"ops[{str(dtype)[6:]},{hd}->{P}]/bwd:{n}", ac.check(f"ops bwd {n}", g, b[n][..., :hd], b["b" + n][..., :hd]))
        ac.check(f"ops bwd_qkv {n}", dqkv[:, :, i].permute(0, 2, 1, 3), b[n][..., :hd], b["b" + n][..., :hd])


def test_wrapper_route(ops, monkeypatch):
    """ops.attention_fwd_qkv takes ldmae_k_norm_max + the bounded kernel iff bf16, head dim <= 32, N >= 512 and B H N^2 >= the threshold."""
    import ldmae_amd.ops as opsmod
    names = []
    real = opsmod.call
    monkeypatch.setattr(opsmod, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    for dtype, hd, N, B, H, thr in ((BF16, 16, 512, 1, 2, 0), (BF16, 32, 512, 1, 2, 2 * 512 * 512), (BF16, 32, 512, 1, 2, 2 * 512 * 512 + 1),
                                    (BF16, 16, 448, 1, 2, 0), (BF16, 64, 512, 1, 2, 0), (F32, 16, 512, 1, 2, 0), (F16, 16, 512, 1, 2, 0)):
        monkeypatch.setattr(opsmod, "BOUNDED_ATTENTION_MIN_SCORES", thr)
        names.clear()
        qkv = torch.randn(B * N, 3 * H * hd, device="cuda").to(dtype)
        ops.attention_fwd_qkv(qkv, B, N, H, hd, hd ** -0.5)
        want = dtype == BF16 and hd <= 32 and N >= 512 and B * H * N * N >= thr
        assert names == (["ldmae_k_norm_max", "ldmae_attention_fwd_qkv_bounded"] if want else ["ldmae_attention_fwd_qkv"]), (dtype, hd, N, thr, names)
