"""CPU: the host side of the patched DDPM (DDPM_2D_patched.py, patch_sampling.py) against the reference's recorded outputs
(tools/make_golden_patched.py -> tests/golden/patched), and a pure-torch restatement of the three box kernels' semantics
(cddpm_box_q_sample, cddpm_box_stitch, cddpm_op_loss_box) that the GPU tests compare the kernels with (tests/test_gpu_patched.py)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, load_pkg

PATCHED = os.path.join(GOLD, "patched")
STITCH_OF = {"p16_paste": "paste", "p12_ragged_paste": "paste", "p12_overlap_cut": "cut", "p12_overlap_avg": "avg"}
SAMPLER_OF = {"p16_paste": dict(patch_size=16), "p12_ragged_paste": dict(patch_size=12),
              "p12_overlap_cut": dict(patch_size=12, overlap=True), "p12_overlap_avg": dict(patch_size=12, overlap=True)}


def patched_golden(name):
    return np.load(os.path.join(PATCHED, name + ".npz"))


# ---- the kernels' semantics in torch (any device). Boxes: integer rows (x0, y1, x2, y3), clipped as Python slicing clips ------------
def box_mask(boxes, H, W):
    """[N,4] -> bool [N,1,H,W]: True inside the clipped box"""
    b = boxes.reshape(-1, 4).long()
    ys = torch.arange(H, device=b.device).view(1, 1, H, 1)
    xs = torch.arange(W, device=b.device).view(1, 1, 1, W)
    c = lambda i: b[:, i].view(-1, 1, 1, 1)
    return (xs >= c(0)) & (xs < c(2)) & (ys >= c(1)) & (ys < c(3))


def ref_box_q_sample(x01, noise, sa_t, s1_t, boxes):
    """N = boxes.shape[0] output slices over S source slices (n reads n % S): 2 x01 - 1 outside the box (exact in fp32), sa (2 x01 - 1) +
    s1 noise inside -- evaluated here in float64: the kernels fuse one product into the sum, so this restatement pins the semantics
    to rounding, and the bits are pinned against the existing q_sample kernel. sa_t, s1_t: [S] coefficients. -> float64"""
    S = x01.shape[0]
    K = boxes.reshape(-1, 4).shape[0] // S
    x0 = (x01 * 2 - 1).double()
    q = sa_t.double().view(-1, 1, 1, 1) * x0 + s1_t.double().view(-1, 1, 1, 1) * noise.double()
    return torch.where(box_mask(boxes, *x01.shape[2:]), q.repeat(K, 1, 1, 1), x0.repeat(K, 1, 1, 1))


def ref_box_stitch(reco, boxes, cut, mode, S):
    """DDPM_2D_patched.py:175-215 as written, with slicing: reco [K S,1,H,W] box-major; -> [S,1,H,W]"""
    N, _c, H, W = reco.shape
    K = N // S
    rows = (cut if mode == "cut" else boxes).reshape(K, S, 4).tolist()
    r = reco.reshape(K, S, 1, H, W)
    out = torch.zeros_like(r[0])
    for k in range(K):
        for j in range(S):
            x0, y1, x2, y3 = rows[k][j]
            if mode == "avg":
                out[j, :, y1:y3, x0:x2] = out[j, :, y1:y3, x0:x2] + r[k, j, :, y1:y3, x0:x2]
            else:
                out[j, :, y1:y3, x0:x2] = r[k, j, :, y1:y3, x0:x2]
        if mode == "avg":          # the reference divides by the FULL mask inside its loop over boxes
            mask = torch.zeros_like(out)
            for kk in range(K):
                for j in range(S):
                    x0, y1, x2, y3 = rows[kk][j]
                    mask[j, :, y1:y3, x0:x2] = mask[j, :, y1:y3, x0:x2] + 1
            out = out / mask
    return out


def ref_loss_box(out, x0, noise, boxes, pred_noise, inpaint, l2, w_b):
    """the loss of p_losses with a box (cond_DDPM.py:612-645) in the dtype of `out` -> per-slice terms [B]; differentiable in `out`"""
    m = box_mask(boxes, *out.shape[2:])
    target = torch.where(m, noise, torch.zeros_like(noise)) if pred_noise else x0
    cmp = torch.where(m, out, x0) if inpaint else out
    d = cmp - target
    per = (d * d if l2 else d.abs()).reshape(out.shape[0], -1).mean(dim=1)
    return per * w_b


# ---- BoxSampler --------------------------------------------------------------------------------------------------------------------
def test_box_sampler_equals_the_reference():
    PS = load_pkg("patch_sampling")
    g = patched_golden("boxes")
    man = json.load(open(os.path.join(PATCHED, "MANIFEST.json")))["boxes"]
    seen = 0
    for key, m in man.items():
        img = torch.zeros(m["batch"], 1, m["H"], m["W"])
        if key.startswith("grid_"):
            bs = PS.BoxSampler(dict(patch_size=m["patch_size"], overlap=m["overlap"]))
            got, cut = bs.sample_grid(img), bs.sample_grid_cut(img)
            assert got.dtype == torch.int64 and tuple(got.shape) == (m["batch"], m["K"], 4)
            assert np.array_equal(got.numpy(), g[key]) and np.array_equal(cut.numpy(), g[key + "_cut"]), key
        else:
            torch.manual_seed(m["seed"])
            bs = PS.BoxSampler(dict(patch_size=m["patch_size"]))
            got = torch.stack([bs.sample_single_box(img) for _ in range(m["draws"])])
            assert tuple(got.shape) == (m["draws"], m["batch"], 4, 1) and np.array_equal(got.numpy(), g[key]), key
        seen += 1
    assert seen == 7
    assert g["grid_32x32_p12_overlap"][0, :3, 0].tolist() == [0, 10, 20]            # positions 0, 10, 20
    assert g["grid_32x32_p12"][0, -1].tolist() == [24, 24, 36, 36]                  # ragged: the last box runs past the edge
    with pytest.raises(ValueError):
        PS.BoxSampler(dict(patch_size=40)).sample_grid(torch.zeros(1, 1, 32, 32))
    with pytest.raises(ValueError):
        PS.BoxSampler(dict(patch_size=40)).sample_single_box(torch.zeros(1, 1, 32, 48))
    assert load_pkg().BoxSampler is PS.BoxSampler                                   # exported by the package


# ---- config ------------------------------------------------------------------------------------------------------------------------
def test_compose_patched_experiment_and_class_selection():
    config = load_pkg("config")
    cfg = config.compose(os.path.join(GOLD, "configs"), "cDDPM/DDPM_patched")
    m = cfg["model"]["cfg"]
    assert cfg["model"]["_target_"] == "src.models.DDPM_2D_patched.DDPM_2D"
    assert m["imageDim"] == [192, 192, 100] and m["rescaleFactor"] == 2 and m["mode"] == "t2"        # ${datamodule.cfg.*} resolved
    assert m["patch_size"] == 48 and m["grid_boxes"] is True and m["inpaint"] is True and m["condition"] is False
    assert m["patch_stride"] == 16 and cfg["trainer"]["precision"] == 32
    cls, patched = config.model_class(cfg["model"]["_target_"])
    assert patched and cls is load_pkg("DDPM_2D_patched").DDPM_2D
    cls, patched = config.model_class("src.models.DDPM_2D.DDPM_2D")
    assert not patched and cls is load_pkg("DDPM_2D").DDPM_2D
    mod = config.instantiate_model(cfg)                       # no device: modules and schedule only
    assert type(mod) is load_pkg("DDPM_2D_patched").DDPM_2D and mod.forward() is None
    assert mod.diffusion.model.image_size == (96, 96) and mod.diffusion.model.num_classes is None
    assert mod.diffusion.model.attention_resolutions == (6, 12, 24)                  # 192 / 32, / 16, / 8: no level
    assert mod.diffusion.inpaint is True and mod.diffusion.objective == "pred_x0" and mod.test_timesteps == 500
    assert mod.boxes.patch_size == 48 and mod.diffusion.sampling_timesteps == 500
    assert not any(k.startswith("encoder.") for k in mod.state_dict())
    with pytest.raises(NotImplementedError):
        config.instantiate_model({"model": {"_target_": "src.models.Spark_2D.Spark_2D", "cfg": {}}})
    with pytest.raises(ValueError):
        config.instantiate_model(cfg, encoder=torch.nn.Identity())


def test_patched_mirror_picks_boxes_as_the_reference_does():
    """training_step / validation_step (:83-91): grid_boxes -> sample_grid then ONE randint over the cells; else sample_single_box"""
    P = load_pkg("DDPM_2D_patched")
    cfg = dict(imageDim=[96, 96, 4], rescaleFactor=3, unet_dim=128, dim_mults=[1, 2, 2], patch_size=12, grid_boxes=True)
    mod = P.DDPM_2D(cfg)
    img = torch.zeros(5, 1, 32, 32)
    torch.manual_seed(11)
    got = mod._pick_boxes(img)
    torch.manual_seed(11)
    ind = torch.randint(0, 9, (5,))
    grid = mod.boxes.sample_grid(img)
    assert tuple(got.shape) == (5, 4, 1) and all(got[j, :, 0].tolist() == grid[j, ind[j]].tolist() for j in range(5))
    mod.cfg["grid_boxes"] = False
    torch.manual_seed(1)
    got = mod._pick_boxes(img[:3])
    assert np.array_equal(got.numpy(), patched_golden("boxes")["single_seed1_B3_32x32_p12"][0])
    assert P.DDPM_2D(dict(cfg, imageDim=[32, 32, 4], rescaleFactor=1)).diffusion.model.attention_resolutions == (1, 2, 4)
    assert P.DDPM_2D(dict(cfg, imageDim=[100, 100, 4], rescaleFactor=1, dim_mults=[1, 2])).diffusion.model.attention_resolutions == (0, 0, 0)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_box_symbols():
    lib_mod = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "cddpm.h")).read()
    declared = set(re.findall(r"\b(cddpm_[a-z0-9_]+)\s*\(", header))
    new = {"cddpm_box_q_sample": 15, "cddpm_box_stitch": 11, "cddpm_op_loss_box": 17}
    lib = lib_mod.load_library()
    for name, nargs in new.items():
        assert name in declared and name in lib_mod.SYMBOLS and hasattr(lib, name), name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == nargs == len(lib_mod.SYMBOLS[name][1]), name
    assert [int(re.search(rf"#define CDDPM_STITCH_{m}\s+(\d+)", header).group(1)) for m in ("PASTE", "CUT", "AVG")] == [0, 1, 2]
    assert load_pkg("engine").CddpmEngine.STITCH_MODES == {"paste": 0, "cut": 1, "avg": 2}


def test_box_rows_accepts_the_reference_shapes():
    E = load_pkg("engine")
    b = torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8]])
    assert E.box_rows(b.unsqueeze(-1), 2).tolist() == b.tolist()                     # [B,4,1], what sample_single_box returns
    assert E.box_rows(b.reshape(2, 1, 4), 2).tolist() == b.tolist()                  # [K,S,4] flattened box-major
    assert E.box_rows(b.tolist()).shape == (2, 4)
    for bad in (b.float(), b[:, :3], b.reshape(-1)):
        with pytest.raises(RuntimeError):
            E.box_rows(bad)
    with pytest.raises(RuntimeError):
        E.box_rows(b, 3)
    with pytest.raises(ValueError):
        E.box_rows(torch.tensor([[-1, 0, 4, 4]]))


# ---- the stitching recurrence against the reference's volumes ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STITCH_OF))
def test_stitch_restatement_equals_the_reference_volume(name):
    """the reference's per-box reconstructions, stitched by ref_box_stitch, give its final_volume bit for bit -- for 'avg' this pins the
    running division (K boxes divide K times), before a GPU sees it"""
    PS = load_pkg("patch_sampling")
    g = patched_golden(name + "__x0_l1_inpaint")
    recos = torch.from_numpy(g["recos"])                       # [K,S,1,H,W]
    K, S, _c, H, W = recos.shape
    bs = PS.BoxSampler(dict(SAMPLER_OF[name]))
    img = torch.zeros(S, 1, H, W)
    boxes, cut = bs.sample_grid(img).permute(1, 0, 2), bs.sample_grid_cut(img).permute(1, 0, 2)      # box-major
    got = ref_box_stitch(recos.reshape(K * S, 1, H, W), boxes, cut, STITCH_OF[name], S)
    vol = torch.from_numpy(g["final_volume"])[0, 0].permute(2, 0, 1).unsqueeze(1)                    # [S,1,H,W]
    assert torch.equal(got, vol)
    if STITCH_OF[name] == "avg":           # and it is NOT the plain mean over the covering boxes
        plain = ref_box_stitch(recos.reshape(K * S, 1, H, W), boxes, cut, "paste", S)
        assert float((got - plain).abs().max()) > 1e-3
