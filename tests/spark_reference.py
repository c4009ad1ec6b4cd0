"""TEST INFRASTRUCTURE: a live torch restatement, dtype-generic and differentiable, of the SparK pre-training forward of the reference
(src/models/Spark_2D.py:26-32; src/models/modules/spark/Spark_2D.py:143-199, encoder.py:13-35, decoder.py:17-76, resnet.py:13-34) for the
one configuration the package builds: resnet50, pyramid 4, BatchNorm densify norms, double = True, heavy [0, 1], cmid 0, no positional
embedding, pix_norm 0, loss on the masked cells. The dense ResNet-50 skeleton is timm's as oracle/encoder_oracle.py restates it; what
SparK does to it is restated operation by operation as the reference writes it: the input and every convolution / pooling output times
the dilated mask, every BatchNorm a BatchNorm1d over the gathered active rows scattered into zeros.

tests/test_spark_reference_host.py ties it to fixtures written by the reference's own code (tools/make_golden_spark.py). The GPU tests
run it in float64 under autograd as the yardstick of the HIP step, with the activation masks of the implementation under test
(act_masks, as encoder_oracle.resnet50_forward takes relu_masks), so that the yardstick differentiates the branch the implementation is on."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

STAGES = ((64, 3), (128, 4), (256, 6), (512, 3))
ENC = "model.sparse_encoder.sp_cnn."
EPS, MOMENTUM = 1e-5, 0.1


def draw_mask(B: int, f: int, mask_ratio: float, generator=None) -> torch.Tensor:
    """SparK_2D.mask with mask_ratio == mask_ratio2 (spark/Spark_2D.py:139-141): bool [B,1,f,f], True = kept; CPU default generator"""
    len_keep = round(f * f * (1 - mask_ratio))
    idx = torch.rand(B, f * f, generator=generator).argsort(dim=1)[:, :len_keep]
    return torch.zeros(B, f * f, dtype=torch.bool).scatter_(dim=1, index=idx, value=True).view(B, 1, f, f)


def dilate(active: torch.Tensor, H: int) -> torch.Tensor:
    r = H // active.shape[-1]
    return active.repeat_interleave(r, 2).repeat_interleave(r, 3)


class _Net:
    def __init__(self, sd, active, training, stats, act_masks, acts):
        self.sd, self.active, self.training, self.stats, self.masks, self.acts = sd, active, training, stats, act_masks, acts

    def _stat(self, p, rows):
        sd = self.sd
        if not self.training:
            return sd[p + ".running_mean"], sd[p + ".running_var"]
        n = rows.shape[0]
        mean, var = rows.mean(0), rows.var(0, unbiased=False)
        if self.stats is not None:
            self.stats[p + ".running_mean"] = (1 - MOMENTUM) * sd[p + ".running_mean"] + MOMENTUM * mean.detach()
            self.stats[p + ".running_var"] = (1 - MOMENTUM) * sd[p + ".running_var"] + MOMENTUM * var.detach() * n / (n - 1)
        return mean, var

    def sparse_bn(self, x, p):
        """sp_bn_forward: BatchNorm1d over the rows of the active pixels, zeros elsewhere"""
        ii = dilate(self.active, x.shape[2]).squeeze(1).nonzero(as_tuple=True)
        bhwc = x.permute(0, 2, 3, 1)
        nc = bhwc[ii]
        mean, var = self._stat(p, nc)
        nc = (nc - mean) / torch.sqrt(var + EPS) * self.sd[p + ".weight"] + self.sd[p + ".bias"]
        out = torch.zeros_like(bhwc).index_put(ii, nc)
        return out.permute(0, 3, 1, 2)

    def dense_bn(self, x, p):
        mean, var = self._stat(p, x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]))
        v = lambda t: t.view(1, -1, 1, 1)
        return (x - v(mean)) / torch.sqrt(v(var) + EPS) * v(self.sd[p + ".weight"]) + v(self.sd[p + ".bias"])

    def masked(self, x):
        return x * dilate(self.active, x.shape[2]).to(x.dtype)

    def _keep(self, y, key):
        if self.acts is not None:
            self.acts[key] = y.detach()
        return y

    def relu(self, t, key):
        return self._keep(F.relu(t) if self.masks is None or key not in self.masks else t * self.masks[key].to(t.dtype), key)

    def relu6(self, t, key):
        if self.masks is None or key not in self.masks:
            return self._keep(F.relu6(t), key)
        mid, high = self.masks[key]
        return self._keep(t * mid.to(t.dtype) + 6.0 * high.to(t.dtype), key)


def spark_forward(x: torch.Tensor, sd: Dict[str, torch.Tensor], active: torch.Tensor, *, loss_on_mask=True, delta_mask=0.0, training=True,
                  drop_scales: Optional[Dict[str, torch.Tensor]] = None, stats: Optional[dict] = None, act_masks: Optional[dict] = None,
                  acts: Optional[dict] = None):
    """x [B,1,H,W], sd: the reference's state dict (model.* names) in x's dtype, active bool [B,1,f,f] -> dict(loss, masked, l1, reco,
    latent, feats = the four masked maps layer1..4). stats: collects the updated running statistics under the state dict's names.
    act_masks: {the ReLU keys of encoder_oracle ("bn1", "<block>.bn1", "<block>.bn2", "<block>.out"): bool [B,C,H,W];
    "dec.<i>": (0 < y < 6, y >= 6); "l1": sign(reco - x) [B,1,H,W], the branch of the L1 term's |.| (its gradient is a sum of +-1 / numel
    over pixels whose signs are as good as random, so one flipped pixel moves every gradient by about 2 / sqrt(numel) of its size)} --
    masks_of() of an activation dict. acts: collects every activation's output (and "l1": reco - x) under those keys."""
    net = _Net(sd, active, training, stats, act_masks, acts)
    B, _c, H, W = x.shape
    f = active.shape[-1]
    p = H // f
    conv = lambda t, name, **kw: F.conv2d(t, sd[name + ".weight"], sd.get(name + ".bias"), **kw)
    # ---- the sparse ResNet-50, pyramid = 4
    h = net.masked(conv(net.masked(x), ENC + "conv1", stride=2, padding=3))
    h = net.relu(net.sparse_bn(h, ENC + "bn1"), "bn1")
    h = net.masked(F.max_pool2d(h, kernel_size=3, stride=2, padding=1))
    feats = []
    for s, (planes, nblocks) in enumerate(STAGES):
        for i in range(nblocks):
            b = f"layer{s + 1}.{i}"
            q = ENC + b
            stride = 2 if (i == 0 and s > 0) else 1
            o = net.relu(net.sparse_bn(net.masked(conv(h, q + ".conv1")), q + ".bn1"), b + ".bn1")
            o = net.relu(net.sparse_bn(net.masked(conv(o, q + ".conv2", stride=stride, padding=1)), q + ".bn2"), b + ".bn2")
            o = net.sparse_bn(net.masked(conv(o, q + ".conv3")), q + ".bn3")
            if training and drop_scales is not None and b in drop_scales:
                o = o * drop_scales[b].to(o.dtype).reshape(-1, 1, 1, 1)
            sc = h
            if i == 0:
                sc = net.sparse_bn(net.masked(conv(h, q + ".downsample.0", stride=stride)), q + ".downsample.1")
            h = net.relu(o + sc, b + ".out")
        feats.append(h)
    latent = feats[-1].mean([2, 3])
    # ---- densify, from the smallest map up
    to_dec = []
    for i, fea in enumerate(reversed(feats)):
        t = net.sparse_bn(fea, f"model.en_de_norms.{i}")
        cur = dilate(active, fea.shape[2])
        t = torch.where(cur.expand_as(t), t, sd[f"model.mask_tokens.{i}"].expand_as(t))
        to_dec.append(conv(t, f"model.en_de_lins.{i}", padding=0 if i == 0 else 1))
    # ---- LightDecoder
    h = 0
    for i in range(5):
        d = f"model.dense_decoder.dec.{i}"
        if i < 4:
            h = h + to_dec[i]
        h = F.conv_transpose2d(h, sd[d + ".up.weight"], sd[d + ".up.bias"], stride=2, padding=1)
        h = net.relu6(net.dense_bn(conv(h, d + ".conv.0.b.0", padding=1), d + ".conv.0.b.1"), f"dec.{i}")
        h = net.dense_bn(conv(h, d + ".conv.0.b.3", padding=1), d + ".conv.0.b.4")
    reco = conv(h, "model.dense_decoder.proj")
    # ---- spatial_loss, pix_norm 0, loss_l2, not dense (spark/Spark_2D.py:180-199); Spark_2D.forward (src/models/Spark_2D.py:26-32)
    non_active = (~active).view(B, -1)
    per_cell = ((reco - x) ** 2).view(B, 1, f, p, f, p).permute(0, 2, 4, 3, 5, 1).reshape(B, f * f, -1).mean(dim=2)
    masked = (per_cell * non_active.to(x.dtype)).sum() / (non_active.sum() + 1e-8)
    if act_masks is not None and "l1" in act_masks:
        l1 = ((reco - x) * act_masks["l1"].to(x.dtype)).mean()          # |d| on a GIVEN branch: sign(d) of the run under test
    else:
        l1 = (reco - x).abs().mean()
    if acts is not None:
        acts["l1"] = (reco - x).detach()
    loss = masked if loss_on_mask else l1 + delta_mask * masked
    return dict(loss=loss, masked=masked, l1=l1, reco=reco, latent=latent, feats=feats)


def masks_of(acts: Dict[str, torch.Tensor]) -> dict:
    """the branch a run is on, from its activation outputs [B,C,H,W]: ReLU -> y > 0; ReLU6 ("dec.<i>") -> (0 < y < 6, y >= 6);
    the L1 term ("l1": reco - x) -> its sign"""
    return {k: ((v > 0) & (v < 6), v >= 6) if k.startswith("dec.") else torch.sign(v) if k == "l1" else v > 0 for k, v in acts.items()}


def to_torch(sd_np, dtype=torch.float64):
    return {k: (torch.from_numpy(v).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v)) for k, v in sd_np.items()}
