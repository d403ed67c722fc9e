"""The 512 x 320 try-on pairs with a change region on the host: the loader of UvitonDatasetFull_512_test on a tiny tree
(tests/tryon_512_tree.py), the restated rules (tests/tryon_512_ref.py) on cases where the rule itself defines the answer, the
45-channel GeneratorFull through pickle, and the command line of pasta-gan_amd/test_512.py.  No GPU."""
import io
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import tryon_512_ref as FR
import tryon_ref as R
from conftest import ROOT
from oracle import param_fill as PF
from oracle import ref_patches as RP
from tryon_512_tree import PAIRS, make_512_tree

CLI = os.path.join(ROOT, 'pasta-gan_amd', 'test_512.py')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_512_tree(tmp_path_factory.mktemp('pairs512'))


def test_loader_reads_the_four_pair_lists_in_order(tree):
    from training.dataset import UvitonDatasetFull_512_test, collate_pairs
    ds = UvitonDatasetFull_512_test(path=tree, change_region='upperbody', use_labels=True, max_size=None, xflip=False)
    assert len(ds) == len(PAIRS) and ds.image_shape == [3, 512, 512] and ds.resolution == 512 and ds.change_region == 'upperbody'
    for i, (sub, person, clothes) in enumerate(PAIRS):
        raw = ds[i]
        assert raw['person_name'] == sub + '/image/' + person and raw['clothes_name'] == sub + '/image/' + clothes
        assert raw['image'].shape == raw['clothes_image'].shape == (512, 320, 3) and raw['image'].dtype == raw['clothes_image'].dtype == np.uint8
        assert raw['parsing'].shape == raw['clothes_parsing'].shape == (512, 320) and raw['parsing'].dtype == np.uint8
        assert raw['keypoints'].dtype == raw['clothes_keypoints'].dtype == np.float64 and raw['keypoints'].shape == (18, 3)
    # <stem>_label.png in all four sub-datasets, MPV included (:1562-1563)
    assert ds._parsing_fnames[4] == os.path.join('MPV_512_320', 'parsing', 'p4_label.png')
    assert ds._clothes_parsing_fnames[4] == os.path.join('MPV_512_320', 'parsing', 'c4_label.png')
    assert ds._clothes_kpt_fnames[2] == os.path.join('Zalora_512_320', 'keypoints', 'c2_keypoints.json')
    assert not ds[3]['keypoints'].any() and not ds[4]['clothes_keypoints'].any()          # empty ``people``
    assert ds[1]['keypoints'][7, 0] < 320 < ds[1]['clothes_keypoints'][7, 0]               # unshifted, as the file has them
    batch = collate_pairs([ds[i] for i in (3, 4)])
    assert tuple(batch['image'].shape) == (2, 512, 320, 3) and tuple(batch['clothes_parsing'].shape) == (2, 512, 320)
    assert tuple(batch['keypoints'].shape) == (2, 18, 3) and batch['keypoints'].dtype.is_floating_point and batch['keypoints'].element_size() == 8
    assert batch['person_name'] == [os.path.join('Deepfashion_512_320', 'image', 'p3.jpg'), os.path.join('MPV_512_320', 'image', 'p4.jpg')]
    assert batch['raw_idx'].tolist() == [3, 4]


def test_loader_refuses_an_unknown_region_at_construction(tree):
    from training.dataset import UvitonDatasetFull_512_test
    from training.tryon_regions import TryOnRegionBatchBuilder
    with pytest.raises(ValueError, match='change region'):
        UvitonDatasetFull_512_test(path=tree, change_region='head')
    with pytest.raises(ValueError, match='change region'):
        TryOnRegionBatchBuilder('cpu', 'head')
    for region in FR.REGIONS:
        assert len(UvitonDatasetFull_512_test(path=tree, change_region=region)) == len(PAIRS)


def test_loader_io_errors(tmp_path):
    import PIL.Image
    from training.dataset import UvitonDatasetFull_512_test
    with pytest.raises(IOError, match='directory'):
        UvitonDatasetFull_512_test(path=str(tmp_path / 'missing'), change_region='fullbody')
    root = make_512_tree(tmp_path / 'tree')
    with pytest.raises(IOError, match='resolution'):
        UvitonDatasetFull_512_test(path=root, change_region='fullbody', resolution=256)
    assert len(UvitonDatasetFull_512_test(path=root, change_region='fullbody', resolution=512)) == len(PAIRS)
    PIL.Image.fromarray(np.zeros([256, 160], np.uint8), mode='L').save(os.path.join(root, 'MPV_512_320', 'parsing', 'c4_label.png'))
    ds = UvitonDatasetFull_512_test(path=root, change_region='fullbody')
    ds[3]
    with pytest.raises(IOError, match='label map'):
        ds[4]
    for sub in ('Zalando_512_320', 'Zalora_512_320', 'Deepfashion_512_320', 'MPV_512_320'):
        open(os.path.join(root, sub, 'test_pairs_front_list_shuffle_0508.txt'), 'w').close()
    with pytest.raises(IOError, match='No image files'):
        UvitonDatasetFull_512_test(path=root, change_region='fullbody')


def test_radius_5_disc_has_69_pixels_and_is_clipped():
    """(r - y)^2 + (c - x)^2 < 25 on integers is skimage's float rule: 81 lattice points within distance 5, less the 12 at
    distance exactly 5."""
    d = FR.disc((40, 30), 20, 15, 5)
    rr, cc = np.mgrid[0:40, 0:30]
    assert d.sum() == 69 and np.array_equal(d, (rr - 20) ** 2 + (cc - 15) ** 2 < 25)
    assert FR.disc((40, 30), 20, 15, 2).sum() == 9
    corner = FR.disc((40, 30), 0, 29, 5)                  # centre on the top-right corner: one quadrant, axes included
    assert np.array_equal(corner, (rr - 0) ** 2 + (cc - 29) ** 2 < 25) and corner.sum() == 22
    assert not FR.disc((40, 30), -6, 10, 5).any()
    pose = np.zeros([18, 3])
    pose[0] = (29.9, 0.2, 1.0)                            # x, y: int() truncation to (29, 0)
    img = FR.draw_pose_from_cords(pose, (40, 30))
    assert np.array_equal(img.any(axis=2), corner) and (img[corner] == R.KPTCOLORS[0]).all()


def test_thickness_5_segments_cover_five_rows_or_columns_plus_caps():
    img = np.zeros([40, 50, 3], np.uint8)
    FR.thick_line(img, (10, 20), (30, 20), (1, 2, 3), 5)              # horizontal, x 10..30 at y 20
    hit = img.any(axis=2)
    assert np.array_equal(np.flatnonzero(hit.any(axis=1)), np.arange(18, 23))
    assert hit[18:23, 10:31].all()
    # caps: 4 d^2 <= 25, d^2 <= 6: beyond the ends (1, 0), (2, 0), (1, +-1), (1, +-2), (2, +-1): 2 columns
    assert np.array_equal(np.flatnonzero(hit.any(axis=0)), np.arange(8, 33))
    assert hit[:, 8].sum() == 3 and hit[:, 9].sum() == 5 and hit[:, 32].sum() == 3 and hit.sum() == 5 * 21 + 2 * 8
    img2 = np.zeros([50, 40, 3], np.uint8)
    FR.thick_line(img2, (20, 10), (20, 30), (1, 2, 3), 5)             # vertical: the transpose
    assert np.array_equal(img2.any(axis=2), hit.T)
    one = np.zeros([20, 20, 3], np.uint8)
    FR.thick_line(one, (10, 10), (10, 10), (9, 9, 9), 5)              # zero length: the disc d^2 <= 6
    assert one.any(axis=2).sum() == 21
    a, b = np.zeros([64, 48, 3], np.uint8), np.zeros([64, 48, 3], np.uint8)
    for p, q in (((3, 5), (40, 60)), ((30, 2), (-8, 50)), ((7, 7), (7, 7))):      # thickness 2 is tests/tryon_ref.py's rule
        FR.thick_line(a, p, q, (5, 6, 7), 2)
        R.thick_line(b, p, q, (5, 6, 7))
    assert np.array_equal(a, b) and a.any()


def test_palm_boxes_of_35_and_20():
    """get_hand_mask :1790, :1795: a k x k box with anchor k // 2 reaches -(k // 2) .. k - 1 - k // 2: -17..17 and -10..9."""
    kp = np.zeros([18, 3])
    kp[[5, 6, 7], :] = [[300, 100, 1], [300, 200, 1], [300, 300, 1]]         # a vertical left arm, already shifted
    for box, rows, reach_lo, reach_hi in ((35, (0, 1), 17, 17), (20, (1, 2), 10, 9)):
        arm = kp[[5, 6, 7]].copy()
        arm[[r for r in range(3) if r not in rows], 2] = 0
        fill = R.get_rectangle_mask(*arm[rows[0], :2], *arm[rows[1], :2], 512, 512) > 0
        up, bottom = FR.hand_masks(arm)
        grown = (up if box == 35 else bottom) > 0
        other = bottom if box == 35 else up
        assert other.all()                                            # the missing segment is an all-ones mask
        cols, rws = np.flatnonzero(fill.any(axis=0)), np.flatnonzero(fill.any(axis=1))
        gcols, grws = np.flatnonzero(grown.any(axis=0)), np.flatnonzero(grown.any(axis=1))
        assert (gcols[0], gcols[-1]) == (cols[0] - reach_hi, cols[-1] + reach_lo)
        assert (grws[0], grws[-1]) == (rws[0] - reach_hi, rws[-1] + reach_lo)
    parsing = np.zeros([512, 512], np.uint8)
    parsing[250:350, 200:400] = 14                                    # a hand across the forearm and beyond the wrist
    palm = FR.palm_mask(kp, parsing)
    assert palm.any() and palm.sum() < (parsing == 14).sum() and not palm[260:290, 290:310].any() and palm[320:350, 200:400].all()


def _two_people():
    """A person and a donor whose garments cannot be confused: different images, the same label map."""
    rng = np.random.default_rng(5)
    lab = np.zeros([512, 320], np.uint8)
    lab[100:200, 50:250], lab[200:230, 50:250], lab[230:260, 50:250] = 5, 6, 7
    lab[300:400, 50:250], lab[400:450, 50:250] = 9, 12
    lab[460:480, 50:250], lab[10:40, 100:200] = 18, 13
    kp = np.zeros([18, 3])
    return dict(image=rng.integers(1, 128, [512, 320, 3], dtype=np.uint8), parsing=lab, keypoints=kp,
                clothes_image=rng.integers(128, 256, [512, 320, 3], dtype=np.uint8), clothes_parsing=lab.copy(), clothes_keypoints=kp)


@pytest.mark.parametrize('region,upper_donor,lower_donor', [('fullbody', True, True), ('upperbody', True, False), ('lowerbody', False, True)])
def test_region_table_picks_the_stated_person(region, upper_donor, lower_donor):
    from training.tryon_regions import REGIONS
    assert FR.region_sources(region) == (upper_donor, lower_donor) == REGIONS[region][1:]
    assert REGIONS[region][0] == FR.REGIONS.index(region)
    raw = _two_people()
    s = FR.label_stages(raw, region)
    pad = lambda a: np.pad(a, ((0, 0), (96, 96), (0, 0)), constant_values=255)
    upper = np.pad(np.isin(raw['parsing'], (5, 6, 7)), ((0, 0), (96, 96)))[..., None]
    lower = np.pad(np.isin(raw['parsing'], (9, 12)), ((0, 0), (96, 96)))[..., None]
    assert np.array_equal(s['upper_img'], upper * pad(raw['clothes_image'] if upper_donor else raw['image']))
    assert np.array_equal(s['lower_img'], lower * pad(raw['clothes_image'] if lower_donor else raw['image']))
    assert np.array_equal(s['upper_mask'], np.repeat(upper, 3, axis=2) * 255) and np.array_equal(s['lower_mask'], np.repeat(lower, 3, axis=2) * 255)
    assert (s['upper_img'][upper[..., 0]] >= 128).all() == upper_donor and (s['lower_img'][lower[..., 0]] >= 128).all() == lower_donor
    keep = np.pad(np.isin(raw['parsing'], (18, 13)), ((0, 0), (96, 96)))[..., None]
    assert np.array_equal(s['retain_img'], keep * pad(raw['image'])) and s['retain_mask'].max() == 1       # always the person's


def test_get_crop_of_the_512_set():
    """No shin fall-back (:1893-1900), the thigh falls back to row 511, key points shifted in float64 first: part_matrices with
    x_pad = 0 and its default shin_fallback equals the restatement; shin_fallback=True (the 256 test set) would keep the shin."""
    from training import patch_pipeline as PP
    rng = np.random.default_rng(1)
    kp = np.concatenate([rng.uniform(0, 500, [3, 18, 2]), rng.uniform(0.2, 1, [3, 18, 1])], axis=2)
    kp[0, 10, 2] = 0.05                                # no right ankle: part 9 invalid
    kp[1, 12, 2] = 0.0                                 # no left knee: thigh from the hip, shin missing
    kp[2, [2, 5], 2] = 0.0                             # no shoulders
    shifted = kp.copy()
    shifted[..., 0] += 96
    fwd, back, valid = PP.part_matrices(shifted, 512, 512, x_pad=0)
    for i in range(3):
        for k, part in enumerate(RP.PARTS):
            m, m_inv = FR.crop_matrices(shifted[i], part, 512, 512)
            assert valid[i, k] == (m is not None), (i, k)
            if m is not None:
                assert np.array_equal(fwd[i, k], m) and np.array_equal(back[i, k], m_inv), (i, k)
    assert not valid[0, 9] and PP.part_matrices(shifted, 512, 512, x_pad=0, shin_fallback=True)[2][0, 9]
    assert valid[1, 6] and not valid[1, 7] and not valid[2, :3].any()
    quad = PP.part_quadrilateral(shifted[1], PP.BODY_PARTS[6], 512, x_pad=0)
    assert quad[2][1] == quad[3][1] == 511.0           # the far end of the fall-back thigh is the last row


def test_generator_full_takes_45_patch_channels_through_pickle():
    from training import networks
    kw = dict(PF.G_KWARGS, synthesis_kwargs=dict(channel_base=256, channel_max=16))
    stem = lambda G: G.style_encoding.model[0].weight.shape[1]
    G45 = networks.GeneratorFull(patch_channels=45, **kw)
    assert stem(G45) == 45 and stem(networks.GeneratorFull(**kw)) == 42 and networks.GeneratorFull.patch_channels == 42
    back = pickle.load(io.BytesIO(pickle.dumps(G45)))
    assert stem(back) == 45 and back.patch_channels == 45 and back.init_kwargs['patch_channels'] == 45
    for (n0, p0), (n1, p1) in zip(G45.state_dict().items(), back.state_dict().items()):
        assert n0 == n1 and p0.shape == p1.shape and bool((p0 == p1).all())


def _cli(*args):
    return subprocess.run([sys.executable, CLI, *args], capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_cli_help_lists_the_reference_options_and_the_region():
    r = _cli('--help')
    assert r.returncode == 0, r.stderr
    for opt in ('--network', '--outdir', '--dataroot', '--batchsize', '--noise-mode', '--trunc', '--seeds', '--class', '--projected-w', '--workers',
                '--change-region', 'fullbody', 'upperbody', 'lowerbody'):
        assert opt in r.stdout, opt


def test_cli_refuses_a_url_and_an_unknown_region(tmp_path):
    r = _cli('--network', 'https://example.com/network-snapshot.pkl', '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path))
    assert r.returncode != 0 and 'URL' in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / 'out').exists()
    r = _cli('--network', str(tmp_path / 'missing.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path))
    assert r.returncode != 0 and 'not a file' in r.stderr
    r = _cli('--network', str(tmp_path / 'missing.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path), '--change-region', 'head')
    assert r.returncode != 0 and 'head' in r.stderr
