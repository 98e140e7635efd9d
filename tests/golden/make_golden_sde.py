#!/usr/bin/env python3
"""Generate tests/golden/sde.npz by IMPORTING THE REFERENCE's transport package and running its own Sampler.sample_sde.

Runs only where the reference checkout is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sde.py

`torchdiffeq` is absent here and the SDE sampler never calls it: a stand-in module with an `odeint` that raises is put into sys.modules before the
import.  Nothing of the reference is copied: the file holds inputs, weights of a toy model defined HERE, and recorded results.

Toy model (analytic, CPU; tests/test_gpu_sde.py restates it on the device):  v = tanh(x W) (1 + t) + b  with W [C, C] acting on the channel
axis, b [C], t [B] broadcast; state [3, 4, 5, 5], num_steps = 6.

Cases: sampling_method in (Euler, Heun) x the six diffusion forms x last_step in (None, Mean, Tweedie, Euler), diffusion_norm 0.7,
last_step_size 0.04, on a reference Transport built directly (linear path, velocity) with sample_eps = 1e-3 -- create_transport forces 0, where
SBDM is infinite at t0 (checked at the end of this script) and where t1 = 1 is singular for last_step None.  Each case runs twice: in f32, and
under torch.set_default_dtype(torch.float64).  th.randn is replaced by a recorder that draws f32 normals from a seeded generator and casts
them to the default dtype, so both runs (and the device run of the test) see the same f32-representable draws; the draws are the same for every
case and are stored once.  The form "constant" hands diffusion_norm over as a 0-dim tensor: with a Python float the reference's own
th.sqrt(2 * diffusion) raises TypeError (sqrt of a float).

Stored:  x0 [3,4,5,5] f32, W, b f32, draws [5,3,4,5,5] f32, norm, last_step_size, sample_eps;
         per case  <case>/traj  [6,3,4,5,5] f64: the reference's f64 trajectory (its returned list, stacked)
                   <case>/dev   [6] f64: max |f32 run - f64 run| per trajectory point (the reference's own f32 error)
                   <case>/t     [6] f32: the grid
         per form  w_<form> [2,6] f64: compute_diffusion at the grid points t (row 0) and at f32(t + dt) (row 1; Heun's second evaluation), for
                   each of the two grids (SBDM's starts at eps) -- keys w_<form>, t_<form>, t2_<form>
                   score_<form> [2,2,6] f64: get_score_from_velocity(v=1, x=0) and (v=0, x=1) at those points: the pair (a, b) of a v + b x
                   (the last point of row 1 lies past t1 and is not used by any step)
"""
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ.setdefault("TORCH_COMPILE_DISABLE", "1")

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/LDMAE"
REAL_RANDN = torch.randn

SHAPE, NUM_STEPS, NORM, LAST_SIZE, EPS = (3, 4, 5, 5), 6, 0.7, 0.04, 1e-3
METHODS = ("Euler", "Heun")
FORMS = ("constant", "SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing")
LAST = (None, "Mean", "Tweedie", "Euler")


def import_reference():
    stub = types.ModuleType("torchdiffeq")

    def odeint(*a, **k):
        raise RuntimeError("the torchdiffeq stand-in: the SDE sampler does not integrate an ODE")
    stub.odeint = odeint
    sys.modules["torchdiffeq"] = stub
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            t = types.ModuleType("tqdm")
            t.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = t
    sys.path.insert(0, REF)
    import transport
    assert transport.__file__.startswith(REF + "/"), transport.__file__
    return transport


def toy_inputs():
    rng = np.random.RandomState(20240607)
    C = SHAPE[1]
    x0 = rng.standard_normal(SHAPE).astype(np.float32)
    W = (rng.standard_normal((C, C)) * 0.6).astype(np.float32)
    b = (rng.standard_normal(C) * 0.3).astype(np.float32)
    return x0, W, b


def toy_model(W, b):
    def model(x, t):
        Wx, bx = W.to(x.dtype), b.to(x.dtype)
        h = torch.tanh(torch.einsum("bchw,cd->bdhw", x, Wx))
        return h * (1 + t.to(x.dtype)).view(-1, 1, 1, 1) + bx.view(1, -1, 1, 1)
    return model


class Recorder:
    """th.randn's stand-in: f32 normals from a seeded generator, cast to the default dtype; every draw is kept."""

    def __init__(self):
        self.gen = torch.Generator().manual_seed(1234)
        self.draws = []

    def __call__(self, *size, **kw):
        size = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else size
        z = REAL_RANDN(size, generator=self.gen, dtype=torch.float32)
        self.draws.append(z.numpy().copy())
        return z.to(torch.get_default_dtype())


def run_case(tp, method, form, last, dtype, x0, W, b):
    torch.set_default_dtype(dtype)
    try:
        tr = tp.Transport(model_type=tp.ModelType.VELOCITY, path_type=tp.PathType.LINEAR, loss_type=tp.WeightType.NONE, train_eps=EPS,
                          sample_eps=EPS, use_cosine_loss=False, use_lognorm=False)
        norm = torch.tensor(NORM) if form == "constant" else NORM
        fn = tp.Sampler(tr).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step=last,
                                       last_step_size=LAST_SIZE, num_steps=NUM_STEPS)
        rec = Recorder()
        torch.randn = rec                                  # the reference calls th.randn, th being torch itself
        try:
            xs = fn(torch.from_numpy(x0).to(dtype), toy_model(torch.from_numpy(W), torch.from_numpy(b)))
        finally:
            torch.randn = REAL_RANDN
        assert len(xs) == NUM_STEPS and all(x.dtype == dtype for x in xs), (len(xs), xs[0].dtype)
        return torch.stack(xs).double().numpy(), np.stack(rec.draws)
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    tp = import_reference()
    path = sys.modules[tp.Transport.__module__].path
    assert path.__file__.startswith(REF + "/")
    x0, W, b = toy_inputs()
    out = dict(x0=x0, W=W, b=b, norm=np.float64(NORM), last_step_size=np.float64(LAST_SIZE), sample_eps=np.float64(EPS))
    draws0 = None
    for method in METHODS:
        for form in FORMS:
            for last in LAST:
                t32, d32 = run_case(tp, method, form, last, torch.float32, x0, W, b)
                t64, d64 = run_case(tp, method, form, last, torch.float64, x0, W, b)
                assert np.array_equal(d32, d64) and d32.shape == (NUM_STEPS - 1,) + SHAPE
                draws0 = d32 if draws0 is None else draws0
                assert np.array_equal(draws0, d32), "the draws differ between cases"
                assert np.isfinite(t64).all() and np.isfinite(t32).all(), (method, form, last)
                case = f"{method}/{form}/{last}"
                out[case + "/traj"] = t64
                out[case + "/dev"] = np.abs(t32 - t64).reshape(NUM_STEPS, -1).max(1)
                lsz = 0.0 if last is None else LAST_SIZE
                t0 = EPS if form == "SBDM" else 0
                t1 = 1 - EPS if lsz == 0 else 1 - lsz
                out[case + "/t"] = torch.linspace(t0, t1, NUM_STEPS).numpy()
                print(f"{case:44s} |x_last| max {np.abs(t64[-1]).max():9.4f}   f32 - f64 per point " + " ".join(f"{v:.1e}" for v in out[case + "/dev"]))
    out["draws"] = draws0
    plan = path.ICPlan()
    for form in FORMS:
        t = torch.linspace(EPS if form == "SBDM" else 0, 1 - LAST_SIZE, NUM_STEPS)
        t2 = t + (t[1] - t[0])
        ws, sc = [], []
        for tt in (t, t2):
            td = tt.double()
            xd = torch.zeros(NUM_STEPS, 1, dtype=torch.float64)
            w = plan.compute_diffusion(xd, td, form=form, norm=torch.tensor(NORM, dtype=torch.float64) if form == "constant" else NORM)
            ws.append((w * torch.ones_like(xd)).reshape(-1).numpy())
            a = plan.get_score_from_velocity(torch.ones_like(xd), torch.zeros_like(xd), td).reshape(-1).numpy()
            bb = plan.get_score_from_velocity(torch.zeros_like(xd), torch.ones_like(xd), td).reshape(-1).numpy()
            sc.append(np.stack([a, bb]))
        out["t_" + form], out["t2_" + form], out["w_" + form], out["score_" + form] = t.numpy(), t2.numpy(), np.stack(ws), np.stack(sc)
    np.savez_compressed(os.path.join(HERE, "sde.npz"), **out)
    print("wrote sde.npz:", os.path.getsize(os.path.join(HERE, "sde.npz")), "bytes,", len(out), "arrays")

    # the default call on a create_transport() transport: SBDM with sample_eps = 0 starts at t0 = 0, where the diffusion is infinite
    tr = tp.create_transport()
    fn = tp.Sampler(tr).sample_sde(num_steps=NUM_STEPS)
    xs = fn(torch.from_numpy(x0), toy_model(torch.from_numpy(W), torch.from_numpy(b)))
    w0 = plan.compute_diffusion(torch.zeros(1, 1), torch.zeros(1), form="SBDM")
    finite = [bool(torch.isfinite(x).all()) for x in xs]
    print(f"reference, default sample_sde() on create_transport(): sample_eps {tr.sample_eps}, compute_diffusion(t=0, 'SBDM') = {float(w0)}, "
          f"finite trajectory points {finite}, non-finite elements of the last {int((~torch.isfinite(xs[-1])).sum())} of {xs[-1].numel()}")
    assert not any(finite), "expected the reference's default SBDM run from t0 = 0 to be non-finite"


if __name__ == "__main__":
    main()
