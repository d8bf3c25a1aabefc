"""GPU: the native training loop -- ClippedAdamW (csrc/optim.h), the Lennard-Jones term (csrc/lj_loss.h), Trainer,
checkpoints and the command line -- against vectors recorded from the reference (tests/golden/make_golden_trainer.py)
and against torch.optim.AdamW + the host restatement of the reference's clipping on the same gradients.

Tolerance rule for everything a HIP kernel computes: the yardstick is the reference's own float32 result against its
float64 result on the same inputs, err_ref = max |f32 - f64| relative to the quantity's largest magnitude; the HIP
result must satisfy |hip - f64| <= 2 err_ref with a floor of 4 float32 ulp of that magnitude, and never exceed 1e-4.
Every comparison prints its figures before it asserts."""
import copy
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests._golden import GOLDEN_DIR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP4 = 4 * 2.0 ** -23


def dev():
    return torch.device("cuda:0")


def _z(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


def within(name, hip, ref64, ref32):
    """The tolerance rule of this file's docstring; -> (err_ref, err_hip), both relative."""
    hip, ref64, ref32 = (torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)).double().reshape(-1)
                         for v in (hip, ref64, ref32))
    mag = max(float(ref64.abs().max()), 1e-30)
    err_ref = float((ref32 - ref64).abs().max()) / mag
    err = float((hip - ref64).abs().max()) / mag
    bound = max(2 * err_ref, ULP4)
    print(f"  {name}: err_ref {err_ref:.3e}  hip {err:.3e}  bound {bound:.3e}  (magnitude {mag:.3e})")
    assert err <= bound and err <= 1e-4, (name, err, bound)
    return err_ref, err


def ref_step(params, grads, opt_sd, queue_items, dtype, lr=1e-3):
    """torch.optim.AdamW + the restated clipping on copies of (params, state, queue) in `dtype`."""
    from diffsbdd_amd.optim import QUEUE_KEY, ReferenceClipper
    ps = [torch.nn.Parameter(p.detach().to(dtype).clone()) for p in params]
    opt = torch.optim.AdamW(ps, lr=lr, amsgrad=True, weight_decay=1e-12)
    if opt_sd is not None:
        sd = copy.deepcopy(opt_sd)
        sd.pop(QUEUE_KEY, None)
        opt.load_state_dict(sd)
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.detach().to(dtype).clone()
    clipper = ReferenceClipper(queue_items)
    norm, max_norm = clipper.clip(ps)
    opt.step()
    return ps, opt, clipper, norm, max_norm


# ---- ClippedAdamW --------------------------------------------------------------------------------------------------------
def test_clipping_and_adamw_follow_the_golden_trace():
    from diffsbdd_amd.optim import ClippedAdamW
    z = _z("trainer_clip")
    shapes = json.loads(str(z["shapes_json"]))
    params = [torch.nn.Parameter(torch.from_numpy(z[f"p0_{i}"]).to(dev())) for i in range(len(shapes))]
    opt = ClippedAdamW(params, lr=1e-3)
    grads = torch.from_numpy(z["grads"]).to(dev())
    n, every = int(z["n_steps"]), int(z["record_every"])
    norms, thrs, entries, clipped = [], [], [], []
    worst = {}
    for k in range(n):
        off = 0
        for p in params[:-1]:
            p.grad = grads[k, off:off + p.numel()].view(p.shape).clone()
            off += p.numel()
        before = [p.grad.clone() for p in params[:-1]]
        opt.step()
        assert all(torch.equal(p.grad, b) for p, b in zip(params[:-1], before))          # p.grad is left unscaled
        rep = opt.clip_report()
        norms.append(rep["last_norm"]); thrs.append(rep["last_max_norm"]); entries.append(rep["queue"][0])
        clipped.append(rep["last_norm"] > rep["last_max_norm"])
        if (k + 1) % every == 0:
            for i, p in enumerate(params):
                views = dict(zip("m v vmax".split(), opt._views(i)))
                for short, val in (("p", p), *views.items()):
                    key = f"step{k + 1}_{short}{i}"
                    if ("f64_" + key) not in z.files:
                        assert i == len(params) - 1 and short != "p"                       # the tensor without a gradient
                        assert float(val.abs().max()) == 0.0
                        continue
                    e = within(key, val, z["f64_" + key], z["f32_" + key])
                    worst[short] = tuple(max(a, b) for a, b in zip(worst.get(short, (0, 0)), e))
    assert clipped == [bool(c) for c in z["f32_clipped"]] and sum(clipped) >= 3             # identical decisions
    worst["norm"] = within("grad norm", np.array(norms), z["f64_norm"], z["f32_norm"])
    worst["threshold"] = within("threshold", np.array(thrs), z["f64_thr"], z["f32_thr"])
    worst["queue entry"] = within("queue entry", np.array(entries), z["f64_entry"], z["f32_entry"])
    print("  worst (err_ref, hip):", {k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in worst.items()})
    assert rep["n_clips"] == sum(clipped) and rep["steps"] == n and len(rep["queue"]) == 50
    assert torch.equal(params[-1].detach().cpu(), torch.from_numpy(z[f"p0_{len(shapes) - 1}"]))   # bit-unchanged
    assert params[-1] not in opt.state and sorted(opt.state_dict()["state"]) == list(range(len(shapes) - 1))


SIZES = [1, 3, 255, 256, 1_000_003, 7]          # the last one has no gradient


@pytest.mark.parametrize("queue", [[1.0, 1.2], [3000.0]], ids=["clipped", "unclipped"])
def test_teacher_forced_single_step_against_torch_adamw(queue):
    from diffsbdd_amd.optim import ClippedAdamW
    g = torch.Generator().manual_seed(3)
    p0 = [torch.randn(n, generator=g).to(dev()) for n in SIZES]
    grads = [[torch.randn(n, generator=g).to(dev()) * (0.5 + k) for n in SIZES[:-1]] + [None] for k in range(3)]
    # two warm-up steps in torch give a non-trivial (p, m, v, vmax, step) to start from
    ps, opt_t, *_ = ref_step(p0, grads[0], None, [3000.0], torch.float32)
    ps, opt_t, *_ = ref_step(ps, grads[1], opt_t.state_dict(), [3000.0], torch.float32)
    start_sd = opt_t.state_dict()
    params = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = ClippedAdamW(params, lr=1e-3)
    from diffsbdd_amd.optim import attach_queue
    opt.load_state_dict(attach_queue(copy.deepcopy(start_sd), queue))
    for p, gr in zip(params, grads[2]):
        p.grad = gr
    opt.step()
    rep = opt.clip_report()
    r32 = ref_step(ps, grads[2], start_sd, queue, torch.float32)
    r64 = ref_step(ps, grads[2], start_sd, queue, torch.float64)
    assert (rep["last_norm"] > rep["last_max_norm"]) == (r32[3] > r32[4]) == (queue != [3000.0])
    within("norm", np.array([rep["last_norm"]]), np.array([r64[3]]), np.array([r32[3]]))
    assert rep["last_max_norm"] == r64[4] and rep["queue"][1:] == r64[2].items[1:]      # two doubles: the same threshold
    within("queue entry", np.array(rep["queue"][:1]), np.array(r64[2].items[:1]), np.array(r32[2].items[:1]))
    for i, n in enumerate(SIZES[:-1]):
        within(f"p[{n}]", params[i], r64[0][i], r32[0][i])
        for k, key in enumerate(("exp_avg", "exp_avg_sq", "max_exp_avg_sq")):
            within(f"{key}[{n}]", opt.state[params[i]][key], r64[1].state[r64[0][i]][key], r32[1].state[r32[0][i]][key])
        assert int(opt.state_dict()["state"][i]["step"]) == 3
    assert torch.equal(params[-1].detach(), ps[-1].detach()) and params[-1] not in opt.state      # None gradient: untouched


def test_plain_optimizer_without_clipping_and_state_dict_exchange_with_torch():
    from diffsbdd_amd.optim import ClippedAdamW, QUEUE_KEY
    g = torch.Generator().manual_seed(4)
    p0 = [torch.randn(n, generator=g).to(dev()) for n in (5, 1030)]
    grads = [torch.randn(n, generator=g).to(dev()) * 50 for n in (5, 1030)]
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = ClippedAdamW(params, clip_grad=False)
    for p, gr in zip(params, grads):
        p.grad = gr
    opt.step()
    sd = copy.deepcopy(opt.state_dict())                   # (a state dict aliases the live state, here as in torch)
    assert QUEUE_KEY not in sd
    r32 = ref_step(p0, grads, None, [1e30], torch.float32)
    r64 = ref_step(p0, grads, None, [1e30], torch.float64)
    for i in range(2):
        within(f"plain p{i}", params[i], r64[0][i], r32[0][i])
    # our state resumes in torch.optim.AdamW, and torch's state resumes here
    t_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    t_opt = torch.optim.AdamW(t_params, lr=1e-3, amsgrad=True, weight_decay=1e-12)
    t_opt.load_state_dict(copy.deepcopy(sd))
    for p, gr in zip(t_params, grads):
        p.grad = gr.clone()
    t_opt.step()
    opt2 = ClippedAdamW([torch.nn.Parameter(p.detach().clone()) for p in params], clip_grad=False)
    opt2.load_state_dict(copy.deepcopy(sd))
    for p, gr in zip(opt2._params, grads):
        p.grad = gr
    opt2.step()
    t64 = ref_step(params, grads, sd, [1e30], torch.float64)
    for i in range(2):
        within(f"resumed p{i}", opt2._params[i], t64[0][i], t_params[i])
    assert int(opt2.state_dict()["state"][0]["step"]) == 2


def _run_steps(n_steps, seed=0):
    from diffsbdd_amd.optim import ClippedAdamW
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, generator=g).to(dev())) for n in (3, 70_001, 512, 9)]
    opt = ClippedAdamW(params, lr=1e-2)
    opt.set_queue([2.0, 2.5])
    for k in range(n_steps):
        for p in params[:-1]:
            p.grad = (torch.randn(p.shape, generator=g) * (4.0 if k % 3 == 0 else 0.01)).to(dev())
        opt.step()
        opt.zero_grad()
    return params, opt


def test_step_makes_no_host_wait_in_the_steady_state():
    params, opt = _run_steps(2)
    grads = [torch.randn_like(p) for p in params[:-1]]
    copies = opt.host_copies
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            for p, gr in zip(params, grads):
                p.grad = gr
            opt.step()
            opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt.host_copies == copies                       # the wrapper read nothing back
    assert opt.clip_report()["steps"] == 5 and opt.host_copies == copies + 1


def test_ten_steps_are_bitwise_reproducible():
    (pa, oa), (pb, ob) = _run_steps(10), _run_steps(10)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    assert torch.equal(oa._flat, ob._flat)
    ra, rb = oa.clip_report(), ob.clip_report()
    assert ra == rb and 0 < ra["n_clips"] < 10 and ra["steps"] == 10
    assert pa[-1] not in oa.state


# ---- Lennard-Jones ---------------------------------------------------------------------------------------------------------
def test_lj_kernel_against_the_golden():
    from diffsbdd_amd.aux_loss import LennardJones
    z = _z("trainer_lj")
    dec = [str(s) for s in z["atom_decoder"]]
    xh = torch.cat([torch.from_numpy(z["x"]), torch.from_numpy(z["h"])], 1).to(dev())
    mask = torch.from_numpy(z["mask"]).to(dev())
    for tag, clamp in (("clamp", 3.0), ("free", None)):
        lj = LennardJones(dec, float(z["norm_value_x"]), clamp, device=dev())
        x = xh.clone().requires_grad_(True)
        u = lj(x, mask, 4)
        (gx,) = torch.autograd.grad(u.sum(), x)
        within(f"lj potential ({tag})", u, z[f"u_{tag}_f64"], z[f"u_{tag}_f32"])
        within(f"lj gradient ({tag})", gx[:, :3], z[f"dx_{tag}_f64"], z[f"dx_{tag}_f32"])
        assert float(gx[:, 3:].abs().max()) == 0.0 and float(u[1]) == 0.0          # argmax: no gradient; one atom: 0
        (g2,) = torch.autograd.grad((lj(x, mask, 4) * torch.tensor([2.0, 1.0, 0.0, -1.0], device=dev())).sum(), x)
        scale = torch.tensor([2.0, 1.0, 0.0, -1.0], device=dev())[mask].unsqueeze(1)
        assert torch.equal(g2[:, :3], gx[:, :3] * scale)                            # backward = a scale per sample


def test_lj_clamped_pair_has_zero_gradient():
    from diffsbdd_amd.aux_loss import LennardJones
    lj = LennardJones("crossdock", 1.0, 3.0, device=dev())
    xh = torch.zeros(5, 13, device=dev())
    xh[:, 3] = 1.0
    xh[1, 0] = 0.3            # sample 0: two carbons 0.3 apart: far above the clamp
    xh[3, 0] = 5.0            # sample 1: two carbons 5 apart: free pair
    mask = torch.tensor([0, 0, 1, 1, 2], device=dev())
    x = xh.clone().requires_grad_(True)
    u = lj(x, mask, 3)
    (gx,) = torch.autograd.grad(u.sum(), x)
    assert float(u[0]) == 6.0 and float(gx[:2].abs().max()) == 0.0
    assert float(u[1]) < 0 and float(gx[2:4, 0].abs().min()) > 0 and float(u[2]) == 0.0


@pytest.mark.parametrize("case", ["loss_small_cond_train", "loss_small_joint_train"])
def test_training_loss_with_the_lj_term_against_the_golden(case):
    """nll_from_terms with the auxiliary term on the stored 12-tuples: the reference's `forward` in float32 / float64."""
    from diffsbdd_amd import train as T
    from diffsbdd_amd.aux_loss import LennardJones, WeightSchedule
    z, g = _z(case), _z("trainer_loss")
    cfg, dd = json.loads(str(z["cfg_json"])), json.loads(str(z["ddpm_json"]))
    names = ("delta_log_px", "error_t_lig", "error_t_pocket", "SNR_weight", "loss_0_x_ligand", "loss_0_x_pocket",
             "loss_0_h", "neg_log_constants", "kl_prior", "log_pN", "t_int_out", "xh_lig_hat")
    terms = [torch.from_numpy(z["out_" + n]).to(dev()) for n in names]
    ligand = {"size": torch.from_numpy(z["ligand_size"]).to(dev()), "mask": torch.from_numpy(z["ligand_mask"]).to(dev())}
    pocket = {"size": torch.from_numpy(z["pocket_size"]).to(dev())}
    aux = (WeightSchedule(dd["timesteps"], 0.001, "linear", device=dev()),
           LennardJones("crossdock", dd["norm_values"][0], 3.0, device=dev()))
    terms[11].requires_grad_(True)
    nll, info = T.nll_from_terms(terms, ligand, pocket, loss_type="l2", training=True, T=dd["timesteps"], x_dims=3,
                                 atom_nf=cfg["atom_nf"], residue_nf=cfg["residue_nf"], aux=aux)
    within("nll with the lj term", nll, g[case + "_lj_nll_f64"], g[case + "_lj_nll"])
    want = float(g[case + "_lj_info_weighted_lj"])
    assert abs(float(info["weighted_lj"]) - want) <= 1e-6 * max(1.0, abs(want))
    (gx,) = torch.autograd.grad(nll.sum(), terms[11])
    assert torch.isfinite(gx).all() and float(gx[:, 3:].abs().max()) == 0.0


# ---- Trainer -----------------------------------------------------------------------------------------------------------------
def small_config(arch="small_cond", tmp="."):
    cfg, dd = W.arch_cfg(arch)
    egnn = {k: cfg[k] for k in ("joint_nf", "hidden_nf", "n_layers", "attention", "tanh", "norm_constant", "inv_sublayers",
                                "normalization_factor", "edge_cutoff_ligand", "edge_cutoff_pocket", "edge_cutoff_interaction",
                                "reflection_equivariant", "edge_embedding_dim")}
    egnn.update(sin_embedding=False, aggregation_method="sum", device="cuda")
    diff = dict(diffusion_steps=dd["timesteps"], diffusion_noise_schedule=dd["noise_schedule"],
                diffusion_noise_precision=dd["noise_precision"], diffusion_loss_type="l2",
                normalize_factors=list(dd["norm_values"]))
    return dict(run_name="run", logdir=str(tmp), dataset="crossdock", datadir=str(tmp), pocket_representation="CA",
                mode="joint" if cfg["update_pocket_coords"] else "pocket_conditioning", batch_size=2, lr=1e-3, n_epochs=10,
                clip_grad=True, auxiliary_loss=False, loss_params=dict(max_weight=0.001, schedule="linear", clamp_lj=3.0),
                egnn_params=egnn, diffusion_params=diff, seed=5, log_every=2, gpus=1)


HIST = np.ones((12, 32))


def complexes():
    from diffsbdd_amd.dataset import ProcessedDataset
    return ProcessedDataset(os.path.join(GOLDEN_DIR, "trainer_complexes.npz"), device=dev())


def _state(tr):
    sd = tr.optimizer.state_dict()
    return ({k: v.detach().cpu().clone() for k, v in tr.ddpm.state_dict().items()},
            {i: {k: torch.as_tensor(v).cpu().clone() for k, v in st.items()} for i, st in sd["state"].items()},
            sd.get("clip_queue"), tr.global_step)


def _same(a, b):
    assert a[3] == b[3] and a[2] == b[2]
    assert a[0].keys() == b[0].keys() and all(torch.equal(a[0][k], b[0][k]) for k in a[0])
    assert a[1].keys() == b[1].keys()
    for i in a[1]:
        assert all(torch.equal(a[1][i][k], b[1][i][k]) for k in a[1][i]), i


def test_trainer_torch_equals_the_loop_written_out(tmp_path):
    from diffsbdd_amd import train as T
    from diffsbdd_amd.dataset import epoch_permutation
    from diffsbdd_amd.optim import ReferenceClipper
    cfg = small_config(tmp=tmp_path)
    ds = complexes()
    tr = T.Trainer(cfg, HIST, ds, None, device=dev(), optimizer="torch")
    tr.fit(max_steps=4)
    # the same four steps from existing pieces
    other = T.Trainer(cfg, HIST, ds, None, device=dev(), optimizer="torch")        # identical initial weights (seeded)
    ddpm = other.ddpm
    params = [p for p in ddpm.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-3, amsgrad=True, weight_decay=1e-12)
    clipper = ReferenceClipper()
    gen = torch.Generator()
    step = 0
    ddpm.train()
    for epoch in range(2):
        order = epoch_permutation(len(ds), cfg["seed"], epoch).tolist()
        for lo in range(0, len(ds), 2):
            if step == 4:
                break
            ddpm.seed(cfg["seed"])
            ddpm._draw = step * T.DRAWS_PER_STEP
            gen.manual_seed(cfg["seed"] * 7919 + step)
            t = torch.randint(0, 21, (2, 1), generator=gen).float()
            ddpm.t_int_source = lambda b, t=t: t
            ligand, pocket = other.ligand_and_pocket(ds.collate(order[lo:lo + 2]))
            terms = ddpm(ligand, pocket, return_info=True)
            nll, _ = T.nll_from_terms(terms, ligand, pocket, loss_type="l2", training=True, T=20, x_dims=3, atom_nf=10,
                                      residue_nf=20)
            nll.mean(0).backward()
            clipper.clip(params)
            opt.step()
            opt.zero_grad(set_to_none=True)
            step += 1
    assert step == 4 and tr.global_step == 4
    for (k, a), b in zip(tr.ddpm.state_dict().items(), ddpm.state_dict().values()):
        assert torch.equal(a, b), k
    assert tr.clipper.items == clipper.items
    rows = [json.loads(line) for line in open(tr.metrics_path)]
    assert [r["step"] for r in rows] == [2, 3, 4]            # log_every = 2, and the end of the 3-batch epoch
    assert all(np.isfinite(r["loss/train"]) for r in rows)


@pytest.mark.parametrize("arch", ["small_cond", "small_joint"])
def test_trainer_hip_teacher_forced_against_torch(arch, tmp_path):
    from diffsbdd_amd import train as T
    from diffsbdd_amd.dataset import epoch_permutation
    cfg = small_config(arch, tmp_path)
    ds = complexes()
    tr = T.Trainer(cfg, HIST, ds, None, device=dev(), optimizer="hip")
    names = [n for n, p in tr.ddpm.named_parameters() if p.requires_grad]
    frozen = {n: p.detach().clone() for n, p in tr.ddpm.named_parameters() if "residue_decoder" in n}
    order = epoch_permutation(len(ds), cfg["seed"], 0).tolist() + epoch_permutation(len(ds), cfg["seed"], 1).tolist()
    for step in range(4):
        p0 = [p.detach().clone() for p in tr.params]
        sd0 = copy.deepcopy(tr.optimizer.state_dict())     # before the step: a state dict aliases the live state
        queue0 = sd0["clip_queue"]["items"]
        tr.ddpm.train()
        tr._key_step(tr.global_step)
        nll, _ = tr.forward(ds.collate(order[2 * step:2 * step + 2]))
        nll.mean(0).backward()
        grads = [None if p.grad is None else p.grad.detach().clone() for p in tr.params]
        tr.optimizer.step()
        r32 = ref_step(p0, grads, sd0 if sd0["state"] else None, queue0, torch.float32)
        r64 = ref_step(p0, grads, sd0 if sd0["state"] else None, queue0, torch.float64)
        worst = (0.0, 0.0)
        for i, n in enumerate(names):
            if grads[i] is None:
                assert torch.equal(tr.params[i].detach(), p0[i]), n
                continue
            hip, a64, a32 = (v.detach().double().cpu() for v in (tr.params[i], r64[0][i], r32[0][i]))
            mag = float(a64.abs().max())
            e_ref, e = float((a32 - a64).abs().max()) / mag, float((hip - a64).abs().max()) / mag
            worst = (max(worst[0], e_ref), max(worst[1], e))
            assert e <= max(2 * e_ref, ULP4) and e <= 1e-4, (n, step, e, e_ref)
        print(f"  {arch} step {step}: worst err_ref {worst[0]:.3e}  hip {worst[1]:.3e}")
        within("queue", np.array(tr.optimizer.clip_report()["queue"]), np.array(r64[2].items), np.array(r32[2].items))
        tr.optimizer.zero_grad()
        tr.global_step += 1
    no_grad = [n for n, g in zip(names, grads) if g is None]
    if arch == "small_cond":                       # pocket-conditioned: the residue decoder never receives a gradient
        assert no_grad and all("residue_decoder" in n for n in no_grad)
        for n, p in tr.ddpm.named_parameters():
            if n in frozen:
                assert torch.equal(p.detach(), frozen[n]), n
        assert all(tr.params[names.index(n)] not in tr.optimizer.state for n in no_grad)
    else:                                          # joint: every decoder trains
        assert not no_grad


def test_resume_is_the_uninterrupted_run(tmp_path):
    from diffsbdd_amd import train as T
    ds = complexes()
    a = T.Trainer(small_config(tmp=tmp_path / "a"), HIST, ds, None, device=dev())
    a.fit(max_steps=8)
    b = T.Trainer(small_config(tmp=tmp_path / "b"), HIST, ds, None, device=dev())
    b.fit(max_steps=4)
    path = b.save_checkpoint()
    step4 = shutil.copy(path, str(tmp_path / "step4.ckpt"))             # (the resumed runs write last.ckpt again)
    del b
    c = T.Trainer.resume(path, ds, None, device=dev())
    assert c.global_step == 4 and c.epoch == 1 and c.batch_in_epoch == 1
    c.fit(max_steps=8)
    _same(_state(a), _state(c))
    ra, rc = a.optimizer.clip_report(), c.optimizer.clip_report()
    assert ra.pop("steps") == 8 and rc.pop("steps") == 4                # (the device counter restarts with the process)
    assert ra == rc
    # and the same from a fresh process: resume the 4-step checkpoint there, train to step 8, compare the files' contents
    code = ("import sys; from diffsbdd_amd import train as T; from diffsbdd_amd.dataset import ProcessedDataset; "
            "ds = ProcessedDataset(sys.argv[2], device='cuda:0'); c = T.Trainer.resume(sys.argv[1], ds, None, device='cuda:0'); "
            "assert c.global_step == 4; c.fit(max_steps=8); print(c.save_checkpoint())")
    run = subprocess.run([sys.executable, "-c", code, step4, os.path.join(GOLDEN_DIR, "trainer_complexes.npz")], cwd=ROOT,
                         capture_output=True, text=True, timeout=180)
    assert run.returncode == 0, run.stderr[-2000:]
    from argparse import Namespace
    with torch.serialization.safe_globals([Namespace]):
        child = torch.load(run.stdout.strip().splitlines()[-1], map_location="cpu", weights_only=True)
    mine = a.checkpoint()
    assert child["global_step"] == mine["global_step"] == 8 and child["clip_queue"] == mine["clip_queue"]
    assert all(torch.equal(child["state_dict"][k], v) for k, v in mine["state_dict"].items())
    so, sm = child["optimizer_states"][0]["state"], mine["optimizer_states"][0]["state"]
    assert so.keys() == sm.keys()
    for i in sm:
        assert all(torch.equal(torch.as_tensor(so[i][k]).cpu(), torch.as_tensor(sm[i][k]).cpu()) for k in sm[i]), i


def test_checkpoint_drives_the_sampler(tmp_path):
    from diffsbdd_amd import train as T
    from diffsbdd_amd.generate import LigandGenerator
    from diffsbdd_amd import synthetic as S
    cfg = small_config(tmp=tmp_path)
    cfg["diffusion_params"]["diffusion_steps"] = 10
    tr = T.Trainer(cfg, HIST, complexes(), None, device=dev())
    tr.fit(max_steps=2)
    path = tr.save_checkpoint()
    gen = LigandGenerator.from_checkpoint(path, device=dev())          # weights_only=True: no trusted=True
    for (k, a), b in zip(gen.ddpm.state_dict().items(), tr.ddpm.state_dict().values()):
        assert torch.equal(a, b), k
    from diffsbdd_amd.molecules import build_molecules
    mem = tr.gen                                           # the generator around the in-memory weights
    mem.ddpm.eval()
    mols = []
    for g in (gen, mem):
        pocket = S.load_pocket("ca", 2, dev())
        g.ddpm.seed(11)
        xh, lig_mask = g.sample_for_pocket(pocket, 2, num_nodes_lig=torch.tensor([6, 8]), timesteps=10)
        x, atom_type, lig_mask = g._drop_virtual(xh, lig_mask)
        mols.append((xh, build_molecules(x, atom_type, lig_mask, g.dataset_info, batch=2)))
    assert torch.equal(mols[0][0], mols[1][0]) and torch.isfinite(mols[0][0]).all()
    assert len(mols[0][1]) == len(mols[1][1]) == 2
    for ma, mb in zip(mols[0][1], mols[1][1]):
        assert ma.symbols == mb.symbols and ma.bonds == mb.bonds and np.array_equal(ma.positions, mb.positions)


def test_command_line_trains_checkpoints_and_lowers_the_loss(tmp_path):
    """`python -m diffsbdd_amd.train` in a child process on the 6-complex file: 10 epochs x 3 batches = 30 steps, seed 5.
    A smoke check, not a measurement: the loss on one fixed (t, noise) batch is lower after the run than before."""
    import yaml
    from diffsbdd_amd import train as T
    data = tmp_path / "data"
    data.mkdir()
    for split in ("train", "val"):
        shutil.copy(os.path.join(GOLDEN_DIR, "trainer_complexes.npz"), data / (split + ".npz"))
    np.save(data / "size_distribution.npy", HIST)
    cfg = small_config(tmp=tmp_path)
    cfg.update(datadir=str(data), logdir=str(tmp_path / "logs"), wandb_params={"mode": "disabled"}, log_every=5)
    (tmp_path / "cfg.yml").write_text(yaml.safe_dump(cfg))
    run = subprocess.run([sys.executable, "-m", "diffsbdd_amd.train", "--config", str(tmp_path / "cfg.yml")], cwd=ROOT,
                         capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stderr[-2000:]
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert summary["global_step"] == 30 and summary["epoch"] == 10
    ckpt_dir = tmp_path / "logs" / "run" / "checkpoints"
    assert (ckpt_dir / "last.ckpt").is_file() and any(f.name.startswith("best-model-epoch=") for f in ckpt_dir.iterdir())
    rows = [json.loads(line) for line in open(summary["metrics"])]
    assert sum("loss/val" in r for r in rows) == 10 and sum("loss/train" in r for r in rows) >= 6
    assert "accepted and ignored" in run.stderr
    again = subprocess.run([sys.executable, "-m", "diffsbdd_amd.train", "--config", str(tmp_path / "cfg.yml"), "--resume",
                            str(ckpt_dir / "last.ckpt")], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert again.returncode == 0, again.stderr[-2000:]                   # resumes at the end of training: nothing left to do
    assert json.loads(again.stdout.strip().splitlines()[-1])["global_step"] == 30
    ds = complexes()
    before = T.Trainer(cfg, HIST, ds, None, device=dev())                # the run's initial weights (same seed)
    after = T.Trainer.resume(str(ckpt_dir / "last.ckpt"), ds, None, device=dev())
    assert after.global_step == 30
    losses = []
    for tr in (before, after):
        tr.ddpm.train()
        tr._key_step(12345)
        with torch.no_grad():
            nll, _ = tr.forward(ds.collate([0, 1, 2, 3, 4, 5]))
        losses.append(float(nll.mean()))
    print("  loss/train on the fixed batch: before %.4f  after 30 steps %.4f" % tuple(losses))
    assert losses[1] < losses[0]
