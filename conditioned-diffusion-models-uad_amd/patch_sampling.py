"""Host-side mirror of the reference's box sampler (reference src/utils/patch_sampling.py): where the patched DDPM
(DDPM_2D_patched.py) noises and reconstructs.

A box is a row (x_min, y_min, x_max, y_max): columns [x_min, x_max) and rows [y_min, y_max). Same constructor keys (`patch_size`,
default 16; `overlap`, default False), the same return shapes and dtypes (int64 on the host) and the same sequence of `torch.randint`
calls as the reference, so under `torch.manual_seed` the random boxes are the reference's. Boxes may run past the right and bottom
edge: whoever applies them clips as Python slicing does (the device kernels of include/cddpm.h do).
"""
from __future__ import annotations

import torch


class BoxSampler:
    def __init__(self, cfg):
        self.patch_size = cfg.get("patch_size", 16)
        self.stride = self.patch_size            # the grid's step: one patch
        self.overlap = cfg.get("overlap", False)

    def _extent(self, image):
        """(batch, height, width, patch width, patch height) after the reference's checks; an int patch_size becomes the pair"""
        batch, _channel, height, width = image.shape
        if isinstance(self.patch_size, int):
            self.patch_size = [self.patch_size, self.patch_size]
        pw, ph = int(self.patch_size[0]), int(self.patch_size[1])
        if ph > height or pw > width:
            raise ValueError("Patch size is larger than image size")
        return batch, height, width, pw, ph

    def sample_single_box(self, image):
        """one random box per image: [batch, 4, 1]. The top-left corner is uniform over the WHOLE image (two randint calls, x first),
        so a box may hang over the right / bottom edge, down to 1 x 1 at the corner."""
        batch, height, width, pw, ph = self._extent(image)
        x_min = torch.randint(0, width, (batch, 1))
        y_min = torch.randint(0, height, (batch, 1))
        return torch.stack((x_min, y_min, x_min + pw, y_min + ph), dim=1)

    def _grid(self, image, spread):
        batch, height, width, pw, ph = self._extent(image)
        xs = torch.arange(0, width, self.stride)
        ys = torch.arange(0, height, self.stride)
        if spread:
            # `overlap`: the same number of patches, their corners spread evenly so that the last one ends at the edge; the positions
            # are floats truncated on assignment into the integer grid (32 wide, patch 12: 0, 10, 20)
            def even(n, extent, patch):
                step = (extent - patch) / (n - 1) if n > 1 else 0.0
                return torch.tensor([int(i * step) for i in range(n)], dtype=xs.dtype)
            xs, ys = even(len(xs), width, pw), even(len(ys), height, ph)
        rows = [torch.stack((x, y, x + pw, y + ph)) for y in ys for x in xs]          # row-major over the grid: y outer, x inner
        return torch.stack(rows).unsqueeze(0).repeat(batch, 1, 1)

    def sample_grid(self, image):
        """the grid of boxes that tiles the image: [batch, K, 4], K = ceil(H / patch) * ceil(W / patch); the last row / column runs past
        the edge when the patch does not divide the image, unless `overlap` spreads the corners evenly"""
        return self._grid(image, bool(self.overlap))

    def sample_grid_cut(self, image):
        """the grid without the overlap adjustment: the cells the 'cut' aggregation pastes each patch's reconstruction into"""
        return self._grid(image, False)
