"""The training run's sample image on the GPU: the reference's ``setup_snapshot_image_grid`` / ``denorm_clothes`` /
``combine_parts`` / ``save_image_grid`` (training/training_loop_wo_flow_fullbody.py:36-209).  A gnum x gnum mix-and-match grid:
row r is a person, column c a clothes donor; with gap = gnum // 3 the first third of the rows swaps the trousers, the second
the whole outfit, the last the top.  The reference warps and erodes every cell on the host (about ten thousand OpenCV calls at
gnum = 23) and keeps fp32 tensors of all cells on the device; here

    setup    the training builder's build(keep_stages=True) of the gnum people, then pasta_grid_composite_eroded_u8 twice
             (upper, lower) for all cells: swap_outfits.grid_composites                    (csrc/train_grid.hip)
    inputs   pasta_grid_assemble: the fp32 tensors G_ema takes, for one minibatch of cells
    save     pasta_image_grid_tile_u8 per minibatch into one uint8 canvas, one copy to the host, PIL writes the PNG

Resident: uint8 only -- the two denormalised images of every cell, the per-person stages, and the canvas frame (side column,
top row)."""

import ctypes
import os

import numpy as np
import PIL.Image
import torch

from torch_utils.ops import _native
from training import patch_pipeline
from training.dataset import collate
from training.swap_outfits import grid_composites
from training.tryon_batch import shift_keypoints

INPUT_KEYS = ['denorm_upper_input', 'denorm_lower_input', 'denorm_upper_mask', 'denorm_lower_mask', 'style_input', 'pose', 'retain']


def cell_sources(gnum):
    """(upper, lower) int arrays [gnum, gnum] indexed [row, col]: whose upper and whose lower patches cell (row, col) wears
    (denorm_clothes :69-84, combine_parts :47-54)."""
    gap = gnum // 3
    row, col = np.meshgrid(np.arange(gnum), np.arange(gnum), indexing='ij')
    return np.where(row < gap, row, col), np.where(row < 2 * gap, col, row)


class SnapshotGrid:
    """``setup`` prepares the grid; ``inputs(lo, hi)`` gives the generator's arguments for cells lo .. hi - 1; ``save`` writes
    an image grid of generated (or any fp32 [n, C, H, H]) images; ``save_init`` the reference's three init_*.png."""

    @classmethod
    def setup(cls, training_set, builder, device, gnum=23):
        vis = list(training_set.vis_index)
        if len(vis) < gnum:
            raise IOError('the snapshot grid needs %d people listed in train_img_vis, the data set has %d' % (gnum, len(vis)))
        raw = collate([training_set[i] for i in vis[:gnum]])       # grid_indices = training_set.vis_index (:113-116)
        from training.tryon_batch import fitted
        raw = fitted(raw, device)                                   # a set opened with ``fit``: the people on their canvas
        if getattr(training_set, 'erase_masks', 'files') == 'strokes':      # drawn by the person: every snapshot shows the same holes
            from training.tryon_batch import attach_strokes
            attach_strokes(raw, training_set.erase_strokes, 0, raw['raw_idx'].numpy())
        return cls(raw, builder.build(raw, keep_stages=True).stages, torch.device(device), gnum, builder)

    def __init__(self, raw, stages, device, gnum, builder):
        self.device, self.gnum, self.cells = device, gnum, gnum * gnum
        image = torch.as_tensor(raw['image']).to(device)
        g, H, W, _ = image.shape
        assert g == gnum
        lp = (H - W) // 2
        self.H = H
        # the padded square of _load_raw_image (dataset.py:520-524)
        self.image = torch.nn.functional.pad(image, (0, 0, lp, H - W - lp), value=255).contiguous()
        self.stick, self.retain_mask = stages['stick'], stages['retain_mask']
        self.norm_img, self.norm_lower = stages['norm_img'], stages['norm_img_lower']

        # Every part is warped with the ROW's M_inv (:86), inverted as cv2.warpPerspective inverts its argument.  These are the
        # float64 matrices normalize_batch inverts, not the float32 copy it returns.  The reference skips a part on
        # M_inv.sum() == 0 (:87), its stand-in for "get_crop found no quadrilateral"; part_matrices' valid flag says that
        # directly (a present matrix whose entries happen to sum to zero is used here and skipped there).
        # The builder says how it formed them: 256 x 192 adds the padding inside get_crop, 512 x 320 shifts the key points first.
        # The grid keeps the host geometry whatever the training batches use.
        keypoints = np.asarray(raw['keypoints'], np.float64)
        if builder.shifted:
            keypoints = shift_keypoints(keypoints, lp)
        maps = patch_pipeline.part_maps(keypoints, H, H, builder.box_factor, builder.x_pad, builder.shin_fallback, self.norm_img.device, 'host')
        upper_src, lower_src = cell_sources(gnum)
        # builder.lower_parts: the parts also cut from the lower garment (:76: 6..9 at 256 x 192)
        self.denorm_upper, self.denorm_lower = grid_composites(stages, maps.back_inv, maps.valid, builder.lower_parts, upper_src, lower_src,
                                                               np.repeat(np.arange(g), g))
        self._frame = {}

    def inputs(self, lo, hi):
        """The generator's keyword arguments (``c`` = style_input) for cells lo .. hi - 1, fp32 NCHW, made by one launch."""
        assert 0 <= lo < hi <= self.cells
        n, H, dev = hi - lo, self.H, self.device
        ph, pw, cu, cl = self.norm_img.shape[1], self.norm_img.shape[2], self.norm_img.shape[3], self.norm_lower.shape[3]
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        t = dict(denorm_upper_input=f32(n, 3, H, H), denorm_lower_input=f32(n, 3, H, H), denorm_upper_mask=f32(n, 1, H, H),
                 denorm_lower_mask=f32(n, 1, H, H), style_input=f32(n, cu + cl, ph, pw), pose=f32(n, 6, H, H), retain=f32(n, 3, H, H))
        outs = (ctypes.c_void_p * 7)(*[t[k].data_ptr() for k in INPUT_KEYS])
        P = _native.ptr
        with torch.cuda.device(dev):
            _native.check(_native.lib().pasta_grid_assemble(P(self.denorm_upper), P(self.denorm_lower), P(self.image), P(self.stick),
                                                            P(self.retain_mask), P(self.norm_img), P(self.norm_lower), outs, lo, n, self.gnum, H,
                                                            ph, pw, cu, cl, _native.stream()))
        t['c'] = t.pop('style_input')
        return t

    def _tile(self, canvas, images, first, gw, ox, oy, drange):
        images = images.to(torch.float32).contiguous()
        _native.require_gpu(images, 'SnapshotGrid.save')
        n, C, H, W = images.shape
        assert canvas.shape[2] == C and (H, W) == (self.H, self.H)
        lo, hi = drange
        with torch.cuda.device(self.device):
            _native.check(_native.lib().pasta_image_grid_tile_u8(_native.ptr(images), _native.ptr(canvas), n, C, H, W, first, gw, ox, oy,
                                                                 int(canvas.shape[0]), int(canvas.shape[1]), float(lo),
                                                                 float(np.float32(255 / (hi - lo))), _native.stream()))

    def frame(self, channels, drange=(-1, 1)):
        """The canvas with its side column and top row (:363-367): the people's own images; the corner is a tile of zeros."""
        key = (channels, tuple(drange))
        if key not in self._frame:
            g, H = self.gnum, self.H
            people = self.image.permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1          # :121
            people = people[:, :channels]
            canvas = torch.empty([(g + 1) * H, (g + 1) * H, channels], dtype=torch.uint8, device=self.device)
            self._tile(canvas, torch.zeros_like(people[:1]), 0, 1, 0, 0, drange)
            self._tile(canvas, people, 0, 1, 0, 1, drange)
            self._tile(canvas, people, 0, g, 1, 0, drange)
            self._frame[key] = canvas
        return self._frame[key].clone()

    def canvas(self, images_by_minibatch, drange=(-1, 1)):
        """uint8 [(gnum + 1) H, (gnum + 1) H, C] on the device from fp32 [n, C, H, H] minibatches covering the cells in order."""
        canvas, first = None, 0
        for images in images_by_minibatch:
            if canvas is None:
                canvas = self.frame(int(images.shape[1]), drange)
            self._tile(canvas, images, first, self.gnum, 1, 1, drange)
            first += int(images.shape[0])
        assert first == self.cells, 'the minibatches cover %d of %d cells' % (first, self.cells)
        return canvas

    def save(self, images_by_minibatch, fname, drange=(-1, 1)):
        array = self.canvas(images_by_minibatch, drange).cpu().numpy()      # the one copy to the host
        if array.shape[2] == 1:
            PIL.Image.fromarray(array[:, :, 0], 'L').save(fname)
        else:
            PIL.Image.fromarray(array, 'RGB').save(fname)

    def save_init(self, run_dir, batch=32):
        """init_denorm_upper.png, init_denorm_lower.png and init_retain.png (:380-386)."""
        for key, name in (('denorm_upper_input', 'init_denorm_upper.png'), ('denorm_lower_input', 'init_denorm_lower.png'),
                          ('retain', 'init_retain.png')):
            self.save((self.inputs(lo, min(lo + batch, self.cells))[key] for lo in range(0, self.cells, batch)), os.path.join(run_dir, name))
