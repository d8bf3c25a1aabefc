"""CPU: the host side of the native training loop against vectors recorded from the reference
(tests/golden/make_golden_trainer.py): dataset + collate, loss assembly, Lennard-Jones radii, clip queue, optimiser
state layout, config refusals, checkpoint format."""
import json
import os
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

from diffsbdd_amd import chem_tables, optim
from diffsbdd_amd import train as T
from diffsbdd_amd.dataset import ProcessedDataset, epoch_permutation
from tests._golden import GOLDEN_DIR


def _z(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


TERM_NAMES = ("delta_log_px", "error_t_lig", "error_t_pocket", "SNR_weight", "loss_0_x_ligand", "loss_0_x_pocket",
              "loss_0_h", "neg_log_constants", "kl_prior", "log_pN", "t_int_out", "xh_lig_hat")


def test_dataset_items_and_collate_equal_the_reference():
    z = _z("trainer_dataset")
    ds = ProcessedDataset(os.path.join(GOLDEN_DIR, "trainer_complexes.npz"))
    assert len(ds) == int(z["n"]) == 6
    for i in range(len(ds)):
        item = ds[i]
        for k in ("lig_coords", "lig_one_hot", "lig_mask", "pocket_coords", "pocket_one_hot", "pocket_mask"):
            assert np.array_equal(item[k].numpy(), z[f"item{i}_{k}"]), (i, k)       # exact: the same float32 arithmetic
        assert int(item["num_lig_atoms"]) == int(z[f"item{i}_num_lig_atoms"])
        assert int(item["num_pocket_nodes"]) == int(z[f"item{i}_num_pocket_nodes"])
    for j, idx in enumerate(json.loads(str(z["lists_json"]))):
        for out in (ds.collate(idx), ds.collate_items([ds[i] for i in idx])):         # device path and host path
            for k in ("lig_coords", "lig_one_hot", "pocket_coords", "pocket_one_hot", "num_lig_atoms", "num_pocket_nodes"):
                assert np.array_equal(out[k].numpy(), z[f"collate{j}_{k}"]), (j, k)
            for k in ("lig_mask", "pocket_mask"):
                assert out[k].dtype == torch.int64 and out[k][0] == 0
                assert np.array_equal(out[k].numpy(), z[f"collate{j}_{k}"].astype(np.int64)), (j, k)
            assert out["names"] == [str(s) for s in z[f"collate{j}_names"]]


def test_dataset_transform_hook_and_epoch_permutation():
    seen = []

    def tf(d):
        seen.append(d["names"])
        d = dict(d)
        d["lig_coords"] = d["lig_coords"] + 1.0
        return d
    path = os.path.join(GOLDEN_DIR, "trainer_complexes.npz")
    plain, hooked = ProcessedDataset(path), ProcessedDataset(path, transform=tf)
    a, b = plain.collate([2, 0]), hooked.collate([2, 0])
    assert seen == ["complex_2", "complex_0"]
    assert torch.equal(b["lig_coords"], a["lig_coords"] + 1.0) and torch.equal(b["pocket_coords"], a["pocket_coords"])
    p0, p0b, p1 = epoch_permutation(6, 4, 0), epoch_permutation(6, 4, 0), epoch_permutation(6, 4, 1)
    assert torch.equal(p0, p0b) and sorted(p0.tolist()) == list(range(6)) and not torch.equal(p0, p1)


@pytest.mark.parametrize("case", ["loss_small_cond_train", "loss_small_cond_eval", "loss_small_joint_train",
                                  "loss_small_joint_eval"])
def test_nll_from_terms_equals_the_reference(case):
    """Element-wise float32 arithmetic in the reference's order on the same CPU kernels: expected exact, and asserted exact."""
    z, g = _z(case), _z("trainer_loss")
    cfg = json.loads(str(z["cfg_json"]))
    training = bool(int(z["training"]))
    terms = [torch.from_numpy(z["out_" + n]) for n in TERM_NAMES]
    info = {k[len("info_"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("info_")}
    ligand = {"size": torch.from_numpy(z["ligand_size"]), "mask": torch.from_numpy(z["ligand_mask"])}
    pocket = {"size": torch.from_numpy(z["pocket_size"])}
    nll, out = T.nll_from_terms((*terms, info), ligand, pocket, loss_type="l2", training=training, T=20, x_dims=3,
                                atom_nf=cfg["atom_nf"], residue_nf=cfg["residue_nf"])
    tag = case + "_plain"
    assert np.array_equal(nll.numpy(), g[tag + "_nll"])
    assert sorted(out) == [str(k) for k in g[tag + "_info_keys"]]
    for k in out:
        assert np.array_equal(torch.as_tensor(out[k]).float().numpy(), g[f"{tag}_info_{k}"]), k
    if not training:                        # outside l2 training the auxiliary term is not added (lightning_modules.py:285)
        assert np.array_equal(g[case + "_lj_nll"], g[tag + "_nll"])


def test_nll_timesteps_come_from_the_golden_config():
    assert json.loads(str(_z("loss_small_cond_eval")["ddpm_json"]))["timesteps"] == 20


def test_lennard_jones_radii_expansion_equals_the_reference():
    z = _z("trainer_lj")
    for name in ("crossdock", "bindingmoad", "crossdock_full"):
        dec = [str(s) for s in z["decoder_" + name]]
        assert dec == chem_tables.dataset_info(name)["atom_decoder"]
        assert np.array_equal(chem_tables.lennard_jones_rm(dec), z["rm_" + name]), name
        assert np.array_equal(chem_tables.lennard_jones_rm(name), z["rm_" + name])


def test_weight_schedule_equals_the_reference():
    from diffsbdd_amd.aux_loss import WeightSchedule
    z = _z("trainer_lj")
    for mode in ("linear", "constant"):
        assert np.array_equal(WeightSchedule(20, 0.001, mode)(torch.arange(21)).numpy(), z["schedule_" + mode])
    with pytest.raises(NotImplementedError):
        WeightSchedule(20, 0.001, "cosine")


def test_host_queue_restatement_equals_the_golden_trace():
    z = _z("trainer_clip")
    for d in ("f32", "f64"):
        clip = optim.ReferenceClipper()
        for k in range(int(z["n_steps"])):
            thr, clipped = clip.decide(float(z[d + "_norm"][k]))
            assert thr == z[d + "_thr"][k] and clipped == bool(z[d + "_clipped"][k]), (d, k)
            assert clip.items[0] == z[d + "_entry"][k]
        assert clip.items == list(z[d + "_queue_final"]) and len(clip.items) == 50
        assert clip.n_clips == int(z[d + "_clipped"].sum()) >= 3


def test_optimizer_state_dict_layout_round_trips_through_torch_adamw():
    """The layout ClippedAdamW writes (torch's own keys + the clip queue) loads into torch.optim.AdamW on CPU; a tensor
    that never had a gradient has no entry."""
    ps = [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2))]
    a = torch.optim.AdamW(ps, lr=1e-3, amsgrad=True, weight_decay=1e-12)
    ps[0].grad, ps[1].grad = torch.randn(3, 2), torch.randn(5)
    a.step()
    sd = optim.attach_queue(a.state_dict(), [1.5, 3000.0], n_clips=0)
    assert sorted(sd["state"]) == [0, 1] and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    assert sd[optim.QUEUE_KEY]["items"] == [1.5, 3000.0]
    b = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1e-3, amsgrad=True, weight_decay=1e-12)
    b.load_state_dict(sd)                                  # the extra key does not disturb torch
    for x, y in zip(ps[:2], b.param_groups[0]["params"][:2]):
        assert torch.equal(a.state[x]["max_exp_avg_sq"], b.state[y]["max_exp_avg_sq"])
    assert b.param_groups[0]["params"][2] not in b.state
    # the param-group keys ClippedAdamW declares cover the ones torch's own groups carry
    ours = {"params", "lr", "betas", "eps", "weight_decay", "amsgrad", *optim.TORCH_GROUP_DEFAULTS}
    assert set(a.param_groups[0]) <= ours, set(a.param_groups[0]) - ours


def test_clipped_adamw_refuses_cpu_and_non_float32_parameters():
    with pytest.raises(Exception, match="GPU only"):
        optim.ClippedAdamW([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(TypeError, match="float32"):
        optim.ClippedAdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="param groups differ"):
        optim.ClippedAdamW([{"params": [torch.nn.Parameter(torch.zeros(3))]},
                            {"params": [torch.nn.Parameter(torch.zeros(3))], "lr": 0.5}])


BASE_CFG = dict(dataset="crossdock", datadir="d", mode="pocket_conditioning", batch_size=4, lr=1e-3, n_epochs=1,
                egnn_params={"hidden_nf": 64}, diffusion_params={"diffusion_steps": 20, "diffusion_loss_type": "l2"})


def test_config_refusals_and_ignored_keys():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cfg = T.check_config(BASE_CFG)
    assert cfg["clip_grad"] is True and cfg["pocket_representation"] == "CA"
    for bad in ({"virtual_nodes": True}, {"augment_noise": 0.1}, {"augment_rotation": True}, {"gpus": 4}):
        with pytest.raises(NotImplementedError):
            T.check_config({**BASE_CFG, **bad})
    with pytest.raises(ValueError, match="batch_size"):
        T.check_config({k: v for k, v in BASE_CFG.items() if k != "batch_size"})
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        T.check_config({**BASE_CFG, "wandb_params": {"mode": "online"}, "visualize_sample_epoch": 5,
                        "eval_params": {"smiles_file": "x"}, "gpus": 1, "augment_noise": 0})
    assert len(w) == 1 and "wandb_params" in str(w[0].message) and "visualize_sample_epoch" in str(w[0].message)
    assert T.check_config({**BASE_CFG, "egnn_params": Namespace(hidden_nf=64)})["egnn_params"] == {"hidden_nf": 64}


def test_load_config_reads_the_reference_yaml_keys(tmp_path):
    yml = tmp_path / "cfg.yml"
    yml.write_text("run_name: 'r'\nlogdir: '%s'\ndataset: 'crossdock'\ndatadir: 'd'\nmode: 'joint'\nbatch_size: 2\n"
                   "lr: 1.0e-3\nn_epochs: 3\ngpus: 1\nclip_grad: True\naugment_rotation: False\naugment_noise: 0\n"
                   "auxiliary_loss: False\nloss_params:\n  max_weight: 0.001\n  schedule: 'linear'\n  clamp_lj: 3.0\n"
                   "egnn_params:\n  hidden_nf: 64\ndiffusion_params:\n  diffusion_steps: 20\n" % tmp_path)
    cfg = T.load_config(str(yml))
    assert cfg["n_epochs"] == 3 and cfg["loss_params"]["clamp_lj"] == 3.0 and cfg["lr"] == 1e-3
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cfg = T.load_config(str(yml), {"lr": 5e-4, "egnn_params": Namespace(hidden_nf=64)})
    assert cfg["lr"] == 5e-4 and any("overwritten" in str(x.message) for x in w)
    yml.write_text(yml.read_text() + "resume: 'x'\n")
    with pytest.raises(ValueError, match="resume"):
        T.load_config(str(yml))


def test_checkpoint_layout_is_read_by_the_sampler_with_weights_only(tmp_path):
    """What save_checkpoint writes: Lightning layout, plain data + argparse.Namespace, `ddpm.` prefix."""
    from diffsbdd_amd.generate import load_checkpoint
    tr = T.Trainer.__new__(T.Trainer)                      # the file format alone: no model, no GPU
    tr.cfg = T.check_config({**BASE_CFG, "loss_params": {"max_weight": 0.001}})
    tr.node_histogram = np.ones((4, 5)).tolist()
    tr.run_dir = str(tmp_path)
    hp = tr.hyper_parameters()
    assert isinstance(hp["egnn_params"], Namespace) and isinstance(hp["diffusion_params"], Namespace)
    p = torch.nn.Parameter(torch.randn(4))
    opt = torch.optim.AdamW([p], amsgrad=True)
    p.grad = torch.randn(4)
    opt.step()
    ck = {"state_dict": {"ddpm.dynamics.w": torch.randn(3)}, "hyper_parameters": hp, "epoch": 1, "global_step": 7,
          "optimizer_states": [optim.attach_queue(opt.state_dict(), [2.0, 3000.0])],
          optim.QUEUE_KEY: {"items": [2.0, 3000.0], "n_clips": 0}}
    path = str(tmp_path / "last.ckpt")
    torch.save(ck, path)
    hp2, sd = load_checkpoint(path)                        # weights_only=True, no trusted=True
    assert list(sd) == ["ddpm.dynamics.w"] and hp2["mode"] == "pocket_conditioning"
    assert hp2["egnn_params"].hidden_nf == 64 and hp2["node_histogram"] == tr.node_histogram
    assert hp2["virtual_nodes"] is False
