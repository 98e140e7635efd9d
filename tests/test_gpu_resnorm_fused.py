"""The gated residuals formed in the norms' row passes (ops.res_rmsnorm_modulate_fwd, ops.rmsnorm_modulate_bwd_gate(recompute=True),
ops.FUSED_RESNORM) against the GEMM-epilogue + norm pair they replace.  Everything here is BITWISE: the row kernels read the branch output
as the GEMM stored it and call the epilogue's own gate_res4, so torch.equal is the only bound.

fp16: the LightningDiT norm kernels are bf16 / f32 only (ops.rmsnorm_modulate_fwd has no fp16 output), so the fp16 reference is the fp16
EPI_GATE_RES GEMM followed by the SAME norm kernel with an f32 output, rounded to fp16 by torch (round-to-nearest-even, what the kernel's own
conversion does)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEPTH, WIDTH, TOKENS = 3, 128, 256


def _randn(shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).cuda()


# ----------------------------------------------------------------------------- y is the same tensor
@pytest.mark.parametrize("K", [768, 2048])
def test_bias_epilogue_and_gate_res_epilogue_store_the_same_y(K):
    from ldmae_amd import ops
    B, rpb, N = 3, 200, 768
    M = B * rpb
    a, w = _randn((M, K), 1, torch.bfloat16), _randn((N, K), 2, torch.bfloat16, K ** -0.5)
    bias, xin, gate = _randn((N,), 3), _randn((M, N), 4), _randn((B, 6 * N), 5)[:, 2 * N:3 * N]
    y_bias = ops.gemm_nt(a, w, bias)
    _, y_gate = ops.gemm_nt_gate_res(a, w, bias, xin, gate, rpb, save_y=True)
    assert y_bias.dtype == y_gate.dtype == torch.bfloat16
    assert torch.equal(y_bias, y_gate)
    assert float(y_bias.float().abs().sum()) > 0


# ----------------------------------------------------------------------------- row kernel against the pair
def _pair_inputs(B, rpb, D, dtype, seed):
    """x, two (a, w, bias) GEMM operand sets whose products are the branch outputs, the [B, 6D] modulation tensor (column slices are the
    strided views the block hands to the kernels) and the norm weight."""
    M, K = B * rpb, 64
    x = _randn((M, D), seed)
    br = [(_randn((M, K), seed + 1 + 3 * i, dtype), _randn((D, K), seed + 2 + 3 * i, dtype, K ** -0.5), _randn((D,), seed + 3 + 3 * i)) for i in range(2)]
    mod = _randn((B, 6 * D), seed + 9, scale=0.5)
    w = 1.0 + _randn((D,), seed + 10, scale=0.1)
    return x, br, mod, w


def _norm_ref(ops, xr, w, sh, sc, rpb, dtype):
    if dtype == torch.bfloat16:
        return ops.rmsnorm_modulate_fwd(xr, w, sh, sc, rpb, dtype)
    out, rstd = ops.rmsnorm_modulate_fwd(xr, w, sh, sc, rpb, torch.float32)       # see the module docstring
    return out.to(dtype), rstd


# (B, rows per sample, D): 3 x 40 -- a workgroup's 16 rows straddle a sample boundary and the last workgroup is ragged (guarded form) at
# D = 768 (3 chunks), 1152 (5 chunks, the last one partial) and 192 (1 partial chunk); 2 x 48 at D = 768 -- the unguarded form (16 | rows per
# sample, 256 | D), which is what the training step runs
SHAPES = [(3, 40, 768), (3, 40, 1152), (3, 40, 192), (2, 48, 768)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("wo_shift", [False, True])
@pytest.mark.parametrize("two", [False, True], ids=["one_residual", "two_residuals"])
@pytest.mark.parametrize("B,rpb,D", SHAPES)
def test_row_kernel_is_the_epilogue_and_norm_pair_bitwise(B, rpb, D, two, wo_shift, dtype):
    from ldmae_amd import ops
    x, br, mod, w = _pair_inputs(B, rpb, D, dtype, 20)
    g1, g2 = mod[:, 2 * D:3 * D], mod[:, 5 * D:6 * D]
    sh, sc = (None if wo_shift else mod[:, 3 * D:4 * D]), mod[:, 4 * D:5 * D]
    # the pair, with the intermediate residual stream materialised
    xr, y1 = ops.gemm_nt_gate_res(br[0][0], br[0][1], br[0][2], x, g1, rpb, save_y=True)
    y2 = None
    if two:
        xr, y2 = ops.gemm_nt_gate_res(br[1][0], br[1][1], br[1][2], xr, g2, rpb, save_y=True)
    xm_ref, rstd_ref = _norm_ref(ops, xr, w, sh, sc, rpb, dtype)
    args = (x, y1, g1, y2, g2 if two else None)
    # every output combination
    xo, xm, rstd = ops.res_rmsnorm_modulate_fwd(*args, w, sh, sc, rpb, want_xout=True, want_norm=True)
    assert torch.equal(xo, xr) and torch.equal(xm, xm_ref) and torch.equal(rstd, rstd_ref)
    xo, xm, rstd = ops.res_rmsnorm_modulate_fwd(*args, w, sh, sc, rpb, want_xout=False, want_norm=True)
    assert xo is None and torch.equal(xm, xm_ref) and torch.equal(rstd, rstd_ref)
    xo, xm, rstd = ops.res_rmsnorm_modulate_fwd(*args, rows_per_batch=rpb, want_xout=True, want_norm=False)
    assert xm is None and rstd is None and torch.equal(xo, xr)
    assert torch.isfinite(xm_ref.float()).all() and float(xm_ref.float().abs().sum()) > 0


def test_row_kernel_rejects_what_it_does_not_implement():
    from ldmae_amd import ops
    x, br, mod, w = _pair_inputs(2, 16, 64, torch.bfloat16, 40)
    y, g = _randn((32, 64), 41, torch.bfloat16), mod[:, :64]
    with pytest.raises(RuntimeError):
        ops.res_rmsnorm_modulate_fwd(x, y, g, w=w, rows_per_batch=16, want_xout=False, want_norm=False)
    with pytest.raises(RuntimeError):
        ops.res_rmsnorm_modulate_fwd(x, y.float(), g, w=w, rows_per_batch=16)
    with pytest.raises(RuntimeError):
        ops.res_rmsnorm_modulate_fwd(x, y, g, w=w, rows_per_batch=5)


# ----------------------------------------------------------------------------- backward variant against the existing kernel
@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("wo_shift", [False, True])
@pytest.mark.parametrize("B,rpb,D", SHAPES)
def test_recomputing_backward_is_the_backward_of_the_stored_row_bitwise(B, rpb, D, wo_shift, accumulate):
    from ldmae_amd import ops
    dtype = torch.bfloat16
    M = B * rpb
    x, br, mod, w = _pair_inputs(B, rpb, D, dtype, 60)
    g1 = mod[:, 2 * D:3 * D]
    sh, sc = (None if wo_shift else mod[:, 3 * D:4 * D]), mod[:, 4 * D:5 * D]
    xmid, y = ops.gemm_nt_gate_res(br[0][0], br[0][1], br[0][2], x, g1, rpb, save_y=True)      # the row as the forward formed it
    _, rstd = ops.rmsnorm_modulate_fwd(xmid, w, sh, sc, rpb, dtype)
    dout, dx0 = _randn((M, D), 70, dtype), _randn((M, D), 71)

    def run(xrow, recompute):
        dx, dmod = dx0.clone(), torch.zeros(B, 6 * D, device="cuda")
        dsh = None if wo_shift else dmod[:, 3 * D:4 * D]
        dw, dy, dbias = ops.rmsnorm_modulate_bwd_gate(dout, xrow, w, sc, rstd, dx, dsh, dmod[:, 4 * D:5 * D], y, g1, dmod[:, 2 * D:3 * D], rpb, dtype,
                                                      accumulate, recompute=recompute)
        return {"dx": dx, "dy": dy, "dmod (dshift, dscale, dgate)": dmod, "dw": dw, "dbias": dbias}
    ref, got = run(xmid, False), run(x, True)
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    assert float(ref["dw"].abs().sum()) > 0 and float(ref["dmod (dshift, dscale, dgate)"][:, 2 * D:3 * D].abs().sum()) > 0


# ----------------------------------------------------------------------------- model level
def _model():
    from ldmae_amd.models.lightningdit import LightningDiT
    torch.manual_seed(0)
    m = LightningDiT(input_size=16, patch_size=1, in_channels=16, hidden_size=WIDTH, depth=DEPTH, num_heads=2, num_classes=10, class_dropout_prob=0.0,
                     use_qknorm=True, use_swiglu=True, use_rope=True, use_rmsnorm=True)
    for mod in [b.adaLN_modulation[1] for b in m.blocks] + [m.final_layer.adaLN_modulation[1], m.final_layer.linear]:      # random non-zero adaLN
        torch.nn.init.normal_(mod.weight, std=0.05)
        torch.nn.init.normal_(mod.bias, std=0.05)
    return m.cuda().train()


@pytest.fixture(scope="module")
def model():
    return _model()


def _step(m, batch, fused, direct=False, hook=False, calls=None):
    """One bf16-autocast training step -> (loss, input gradient, parameter gradients); `calls` counts the row-kernel launches of the forward."""
    from ldmae_amd import ops
    x, t, y = _randn((batch, 16, 16, 16), 100).requires_grad_(True), torch.linspace(0.1, 0.9, batch).cuda(), (torch.arange(batch) % 10).cuda()
    target = _randn((batch, 16, 16, 16), 101)
    real = ops.res_rmsnorm_modulate_fwd

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    handle = m.blocks[1].register_forward_hook(lambda mod, i, o: None) if hook else None
    ops.FUSED_RESNORM = fused
    if calls is not None:
        ops.res_rmsnorm_modulate_fwd = counted
    try:
        m.direct_param_grads = direct
        for p in m.parameters():
            p.grad = torch.zeros_like(p) if direct else None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(x, t, y)
        loss = ((out.float() - target) ** 2).mean()
        loss.backward()
        return loss.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    finally:
        ops.FUSED_RESNORM = True
        ops.res_rmsnorm_modulate_fwd = real
        m.direct_param_grads = False
        if handle is not None:
            handle.remove()


def _assert_same_step(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].keys() == b[2].keys() and len(a[2]) > 30
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    assert torch.isfinite(a[0]) and float(a[1].abs().sum()) > 0 and float(a[2]["blocks.1.norm2.weight"].abs().sum()) > 0


@pytest.mark.parametrize("direct", [False, True], ids=["autograd_grads", "direct_param_grads"])
def test_training_step_is_bitwise_the_step_of_the_epilogue_path(model, direct):
    on_calls, off_calls = [], []
    on = _step(model, 8, True, direct=direct, calls=on_calls)
    off = _step(model, 8, False, direct=direct, calls=off_calls)
    assert len(on_calls) == 2 * DEPTH and len(off_calls) == 0         # row pass 1 and row pass 2 of every block; none with the switch off
    _assert_same_step(on, off)


def test_hooked_block_takes_the_fallback(model):
    calls = []
    on = _step(model, 8, True, hook=True, calls=calls)
    assert len(calls) == 0                                             # a hook on block 1: no chain, so no hand-off and no fused row pass
    _assert_same_step(on, _step(model, 8, False, hook=True))


def _block_nodes(fn):
    seen, todo, found = set(), [fn], []
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        if type(n).__name__ == "_DiTBlockFnBackward":
            found.append(n)
        todo.extend(f for f, _ in n.next_functions)
    return found


def test_batch_without_batched_adaln_keeps_todays_saved_tensors(model):
    """Batch 2: no mod_all, so the block takes today's path whatever the switch says, with today's ctx.saved_tensors (29 entries; x2 first,
    the stored mid-block residual stream -- a buffer of its own -- in slot 14, then rstd2)."""
    calls = []
    _assert_same_step(_step(model, 2, True, calls=calls), _step(model, 2, False))
    assert len(calls) == 0
    x, t, y = _randn((2, 16, 16, 16), 100).requires_grad_(True), torch.tensor([0.3, 0.7]).cuda(), torch.tensor([1, 2]).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(x, t, y)
    nodes = _block_nodes(out.grad_fn)
    assert len(nodes) == DEPTH
    M = 2 * TOKENS
    for n in nodes:
        sv = n.saved_tensors
        assert len(sv) == 29
        x2, y1, xmid, rstd2 = sv[0], sv[13], sv[14], sv[15]
        assert x2.shape == (M, WIDTH) and x2.dtype == torch.float32
        assert y1.shape == (M, WIDTH) and y1.dtype == torch.bfloat16
        assert xmid.shape == (M, WIDTH) and xmid.dtype == torch.float32 and xmid.data_ptr() != x2.data_ptr()
        assert rstd2.shape == (M,)


def test_mid_block_residual_stream_is_not_stored(model):
    """Peak memory over forward + backward drops by the mid-block residual stream of every block (depth x M x D x 4 bytes expected; at least
    half of it required, so allocator rounding cannot hide a regression)."""
    def peak(fused):
        _step(model, 8, fused)                                         # warm: workspaces and cached weight copies exist
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        _step(model, 8, fused)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()
    p_on, p_off = peak(True), peak(False)
    want = DEPTH * 8 * TOKENS * WIDTH * 4
    print(f"peak allocated: fused {p_on} B, epilogue path {p_off} B, drop {p_off - p_on} B (expected {want} B)")
    assert p_off - p_on >= want // 2
