"""The inputs that ops.py legitimately copies or converts (tests/test_ops_args_cpu.py: ALLOWED_ON's COPIED and CONVERTED) give the bits of the
dense / float32 input, and what no copy can mend -- another type, a shape that disagrees -- is refused before anything is launched.  One wave or
one tile per call."""
import pytest
import torch

from ldmae_amd import ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def rnd(*shape, seed=0, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def strided(t):
    """A non-contiguous view with the shape and values of t (every other column of a tensor twice as wide)."""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    wide[..., ::2] = t
    v = wide[..., ::2]
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


def test_silu_bwd_strided_dy():
    dy, x = rnd(2, 8, seed=1), rnd(2, 8, seed=2)
    assert torch.equal(ops.silu_bwd(strided(dy), x), ops.silu_bwd(dy, x))
    with pytest.raises(RuntimeError, match="silu_bwd x: dtype"):
        ops.silu_bwd(dy, x.half())
    with pytest.raises(RuntimeError, match="silu_bwd dy: shape"):
        ops.silu_bwd(rnd(2, 16), x)


def test_rope_strided_t():
    t, cos, sin = rnd(1, 2, 16, seed=1), rnd(2, 16, seed=2), rnd(2, 16, seed=3)
    out = ops.rope(strided(t), cos, sin)
    assert out.is_contiguous() and torch.equal(out, ops.rope(t, cos, sin))
    with pytest.raises(RuntimeError, match="rope sin: shape"):
        ops.rope(t, cos, sin[:, :8])
    with pytest.raises(RuntimeError, match="rope t: dtype"):
        ops.rope(t.half(), cos, sin)


@pytest.mark.parametrize("H", [1, 2])            # one head; two heads: the smallest shape at which a permuted q is no dense tensor
def test_attention_bwd_strided_do_and_refusals_launch_nothing(H):
    B, N, hd = 1, 64, 32
    q, k, v = (rnd(B, H, N, hd, seed=s, dtype=BF16) for s in (1, 2, 3))
    o, lse = ops.attention_fwd(q, k, v, hd ** -0.5)
    do = rnd(B, N, H * hd, seed=4, dtype=BF16)
    want = ops.attention_bwd(q, k, v, o, do, lse, hd ** -0.5)
    got = ops.attention_bwd(q, k, v, o, strided(do), lse, hd ** -0.5)
    assert all(g.is_contiguous() and torch.equal(g, w) for g, w in zip(got, want))
    # a permuted q ([B, N, H, hd] storage seen as [B, H, N, hd]): copied, and dq / dk / dv come out dense, not in q's strides
    qp = q.transpose(1, 2).contiguous().transpose(1, 2)
    assert qp.is_contiguous() == (H == 1) and torch.equal(qp, q)
    got = ops.attention_bwd(qp, k, v, o, do, lse, hd ** -0.5)
    assert all(g.is_contiguous() and torch.equal(g, w) for g, w in zip(got, want))
    torch.cuda.synchronize()
    before = ops.launch_counts()
    with pytest.raises(RuntimeError, match="attention_bwd k: shape"):          # q taken as [B, N, H, hd]: the others disagree with it
        ops.attention_bwd(q.transpose(1, 2), k, v, o, do, lse, hd ** -0.5)
    with pytest.raises(RuntimeError, match="attention_bwd lse: shape"):
        ops.attention_bwd(q, k, v, o, do, lse[..., :32], hd ** -0.5)
    with pytest.raises(RuntimeError, match="attention_bwd do: dtype"):
        ops.attention_bwd(q, k, v, o, do.float(), lse, hd ** -0.5)
    assert ops.launch_counts() == before


def test_random_masking_strided_noise():
    noise = torch.rand(2, 16, generator=torch.Generator().manual_seed(5)).cuda()
    want, got = ops.random_masking(noise, 4), ops.random_masking(strided(noise), 4)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    with pytest.raises(RuntimeError, match="random_masking noise: dtype"):
        ops.random_masking(noise.double(), 4)


def test_latent_prologue_bf16_moments():
    mom, noise = rnd(1, 4, 2, 2, seed=6, dtype=BF16), rnd(1, 2, 2, 2, seed=7)
    mean, std = rnd(2, seed=8), rnd(2, seed=9).abs() + 0.5
    assert torch.equal(ops.latent_prologue(mom, noise, mean, std), ops.latent_prologue(mom.float(), noise, mean, std))
    with pytest.raises(RuntimeError, match="latent_prologue noise: shape"):
        ops.latent_prologue(mom, rnd(1, 4, 2, 2), mean, std)
    with pytest.raises(RuntimeError, match="latent_prologue lat_std: shape"):
        ops.latent_prologue(mom, noise, mean, rnd(4))
