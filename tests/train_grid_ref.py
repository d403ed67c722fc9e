"""numpy restatement of the reference training loop's sample grid (training/training_loop_wo_flow_fullbody.py): ``combine_parts``
:36-56, ``denorm_clothes`` :59-107, ``setup_snapshot_image_grid`` :109-178, the side column and top row :363-367 and
``save_image_grid`` :182-203.  The kernels of csrc/train_grid.hip and training/snapshot_grid.py are held to it bit for bit
(tests/test_train_grid_gpu.py, tests/test_train_run_gpu.py).

Built from oracle/ref_patches.py's ``warp_perspective`` / ``part_transforms`` / ``normalize``, tests/tryon_ref.py's
``label_masks`` and tests/tryon_pairs_ref.py's brute-force ``erode``.  Parity with OpenCV itself is UNPINNED, as for every other
warp here.  Two decisions of the project are restated, not the reference's letter: the warp-back matrices are the float64
ones get_crop computes (the reference passes the float32 copy its data set returns), and a part is skipped when get_crop
found no quadrilateral (the reference tests M_inv.sum() == 0)."""
import numpy as np
import torch

import tryon_ref as R
from oracle import ref_patches as RP
from tryon_pairs_ref import erode


def combine_parts(parts, col, row, gnum):
    """:36-56 on [g, 42, h, w]: 30 upper channels, 12 lower."""
    col_part, row_part = parts[col], parts[row]
    gap = gnum // 3
    if row < gap:                       # trousers swapped
        return np.concatenate([row_part[:30], col_part[30:]], axis=0)
    if row < 2 * gap:                   # whole outfit
        return col_part
    return np.concatenate([col_part[:30], row_part[30:]], axis=0)     # top swapped


def denorm_from(norm_patches, norm_patches_lower, m_invs, masks, masks_lower, upper_src, lower_src, row):
    """The body of denorm_clothes (:60-107) for a cell whose upper patches are person upper_src's and whose lower patches are
    person lower_src's: every part back with m_invs[row], every mask eroded 5 x 5 before the == 255 test."""
    size = 256
    den_u, den_l = np.zeros((size, size, 3), np.uint8), np.zeros((size, size, 3), np.uint8)
    skipped = 0
    for ii in range(len(m_invs[row])):
        m_inv = m_invs[row][ii]
        if m_inv is None:
            skipped += 1
            continue
        patch = norm_patches[upper_src, ii * 3:(ii + 1) * 3].transpose(1, 2, 0)
        mask = masks[upper_src, ii * 3:(ii + 1) * 3].transpose(1, 2, 0)
        back = RP.warp_perspective(np.ascontiguousarray(patch), m_inv, (size, size), RP.BORDER_CONSTANT)
        back_mask = RP.warp_perspective(np.ascontiguousarray(mask), m_inv, (size, size), RP.BORDER_CONSTANT)
        hit = (erode(back_mask, 5)[..., 0:1] == 255).astype(np.uint8)
        den_u = back * hit + den_u * (1 - hit)
        if ii >= 6:
            patch = norm_patches_lower[lower_src, (ii - 6) * 3:(ii - 5) * 3].transpose(1, 2, 0)
            mask = masks_lower[lower_src, (ii - 6) * 3:(ii - 5) * 3].transpose(1, 2, 0)
            back = RP.warp_perspective(np.ascontiguousarray(patch), m_inv, (size, size), RP.BORDER_CONSTANT)
            back_mask = RP.warp_perspective(np.ascontiguousarray(mask), m_inv, (size, size), RP.BORDER_CONSTANT)
            hit = (erode(back_mask, 5)[..., 0:1] == 255).astype(np.uint8)
            den_l = back * hit + den_l * (1 - hit)
    return den_u, den_l, skipped


def cell_sources(col, row, gnum):
    """(upper, lower): whose patches cell (row, col) wears (:69-84)."""
    gap = gnum // 3
    return (row if row < gap else col), (col if row < 2 * gap else row)


def denorm_clothes(norm_patches, norm_patches_lower, m_invs, masks, masks_lower, col, row, gnum):
    """:59-107 -> (upper [1,3,H,H], lower, upper mask [1,1,H,H], lower mask) uint8, and the number of skipped parts."""
    upper_src, lower_src = cell_sources(col, row, gnum)
    den_u, den_l, skipped = denorm_from(norm_patches, norm_patches_lower, m_invs, masks, masks_lower, upper_src, lower_src, row)
    den_u, den_l = den_u.transpose(2, 0, 1)[np.newaxis], den_l.transpose(2, 0, 1)[np.newaxis]
    mask_u = (np.sum(den_u, axis=1, keepdims=True) > 0).astype(np.uint8)
    mask_l = (np.sum(den_l, axis=1, keepdims=True) > 0).astype(np.uint8)
    return den_u, den_l, mask_u, mask_l, skipped


def people(samples):
    """What training_set[i] returns for the listed people (dataset.py:515-568, 929-993), as far as the grid reads it, stacked:
    CHW uint8 arrays and, per person, the ten float64 M_inv (None where get_crop found no quadrilateral)."""
    out = dict(images=[], poses=[], norm_img=[], norm_img_lower=[], masks=[], masks_lower=[], retain_masks=[], m_invs=[])
    for s in samples:
        image, pose, retain, _, ui, li, um, lm, _ = R.label_masks(s['image'], s['parsing'], s['keypoints'])
        ni, nl, _, _, _, _, cm, cml = RP.normalize(ui, li, um, lm, s['keypoints'])
        out['images'].append(image.transpose(2, 0, 1))
        out['poses'].append(pose.transpose(2, 0, 1))
        out['norm_img'].append(ni.transpose(2, 0, 1))
        out['norm_img_lower'].append(nl.transpose(2, 0, 1))
        out['masks'].append(cm.transpose(2, 0, 1))
        out['masks_lower'].append(cml.transpose(2, 0, 1))
        out['retain_masks'].append(retain[None])
        out['m_invs'].append([m_inv for _, m_inv in RP.part_transforms(s['keypoints'], image.shape[1], image.shape[0])])
    return {k: (v if k == 'm_invs' else np.stack(v)) for k, v in out.items()}


def setup_snapshot_image_grid(samples, gnum):
    """:109-178 up to the float conversions: the people's arrays plus denorm_upper / denorm_lower [gnum^2, 3, H, H] and their
    masks [gnum^2, 1, H, H] (uint8) for cell i = (row i // gnum, col i % gnum), and the skipped-part count per cell."""
    p = people(samples[:gnum])
    cells = [denorm_clothes(p['norm_img'], p['norm_img_lower'], p['m_invs'], p['masks'], p['masks_lower'], i % gnum, i // gnum, gnum)
             for i in range(gnum * gnum)]
    names = ('denorm_upper', 'denorm_lower', 'denorm_upper_mask', 'denorm_lower_mask')
    grid = {name: np.concatenate([c[k] for c in cells], axis=0) for k, name in enumerate(names)}
    grid['skipped'] = [c[4] for c in cells]
    grid['parts'] = np.concatenate([p['norm_img'], p['norm_img_lower']], axis=1)      # :149-150
    grid.update(p)
    return grid


def person_tensors(grid, device):
    """images, poses (6 channels) and retain of the people, the loop's expressions evaluated by torch on ``device`` (:121, :160-168)."""
    images = torch.from_numpy(grid['images']).to(device).to(torch.float32) / 127.5 - 1
    poses = torch.from_numpy(grid['poses']).to(device).to(torch.float32) / 127.5 - 1
    retain_masks = torch.from_numpy(grid['retain_masks']).to(device)
    retain = retain_masks * images - (1 - retain_masks)
    return images, torch.cat((poses, retain), dim=1), retain


def generator_inputs(grid, gnum, lo, hi, device):
    """The tensors of cells lo .. hi - 1 as the reference's loop holds them (:132-175), evaluated by torch on ``device``."""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device).to(torch.float32)
    _, poses, retain = person_tensors(grid, device)
    parts = f(grid['parts']) / 127.5 - 1
    parts_np = parts.cpu().numpy()
    cells = range(lo, hi)
    style = torch.from_numpy(np.stack([combine_parts(parts_np, i % gnum, i // gnum, gnum) for i in cells])).to(device)
    rows = [i // gnum for i in cells]
    return dict(denorm_upper_input=f(grid['denorm_upper'][lo:hi]) / 127.5 - 1, denorm_lower_input=f(grid['denorm_lower'][lo:hi]) / 127.5 - 1,
                denorm_upper_mask=f(grid['denorm_upper_mask'][lo:hi]), denorm_lower_mask=f(grid['denorm_lower_mask'][lo:hi]),
                c=style, pose=poses[rows], retain=retain[rows])


def frame(source_im):
    """:363-367 from the people's fp32 images [g, C, H, W] (numpy): (image_side [g H, W, C], image_top [H, (g + 1) W, C])."""
    g, C, H, W = source_im.shape
    image_side = source_im[:, None].transpose(0, 3, 1, 4, 2).reshape(g * H, W, C)
    image_top = np.concatenate((np.zeros((1, C, H, W), source_im.dtype), source_im), axis=0)
    image_top = image_top[None].transpose(0, 3, 1, 4, 2).reshape(H, (g + 1) * W, C)
    return image_side, image_top


def save_image_grid(im_side, im_top, img, drange, grid_size):
    """:182-203 without the file: the uint8 array that PIL is given."""
    lo, hi = drange

    def to_u8(a):
        a = np.asarray(a, dtype=np.float32)
        a = (a - lo) * (255 / (hi - lo))
        with np.errstate(invalid='ignore'):
            return np.rint(a).clip(0, 255).astype(np.uint8)
    nan = np.isnan(np.asarray(img, dtype=np.float32))
    img, im_side, im_top = to_u8(img), to_u8(im_side), to_u8(im_top)
    img[nan] = 0                        # numpy leaves the conversion of a NaN undefined; the kernel's answer is 0
    gw, gh = grid_size
    _N, C, H, W = img.shape
    img = img.reshape(gh, gw, C, H, W).transpose(0, 3, 1, 4, 2).reshape(gh * H, gw * W, C)
    img = np.concatenate((im_side, img), axis=1)
    return np.concatenate((im_top, img), axis=0)
