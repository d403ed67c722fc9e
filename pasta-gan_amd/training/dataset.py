"""The try-on training data set of the reference (training/dataset.py: ``Dataset`` :54-185, ``UvitonDatasetFull`` :426-995),
reading the same directory layout with PIL and ``json`` only.

Difference from the reference, by design: ``UvitonDatasetFull.__getitem__`` returns the RAW sample -- the decoded files -- and
not the prepared 13-tuple.  The preparation (stick figure, palm / retain masks, garment images and masks, body-part warps, erase
mask, float conversions) runs for a whole batch on the GPU in ``training.tryon_batch.FullBodyBatchBuilder``; ``collate`` turns
a list of raw samples into the batch the builder takes.  Only directory data sets are supported, as in the reference.
The test pairs (``UvitonDatasetV19_test``, dataset.py:997-1525) follow the same design: raw pairs out, ``collate_pairs``, and
``training.tryon_pairs.TryOnPairBatchBuilder`` on the GPU; so do the 512 x 320 pairs with a change region
(``UvitonDatasetFull_512_test``, dataset.py:1528-2214) with ``training.tryon_regions.TryOnRegionBatchBuilder``.
``UvitonOutfits_512_test`` is this project's own: outfits (person, upper garment's donor, lower garment's donor) from a list
file, ``collate_outfits`` and ``training.tryon_regions.TryOnOutfitBatchBuilder``.
``UvitonDatasetFull_512`` is this project's own: the training layout at 512 x 320, which the reference does not ship, prepared
by ``training.tryon_regions.FullBodyRegionBatchBuilder``.
Every class takes ``fit='pad' | 'crop'`` (this project's own): the files may then have any size, samples keep it, the collate
functions pack them instead of stacking (``pack_people``), and the builders fit them to the class's ``canvas`` on the GPU
(``training.tryon_batch.fit_batch``; include/pasta_hip.h has the rule)."""

import json
import os

import numpy as np
import PIL.Image
import torch

SUB_DATASETS = ('Zalando_256_192', 'Zalora_256_192', 'Deepfashion_256_192', 'MPV_256_192')     # dataset.py:435
PAIR_LIST = 'train_pairs_front_list_0508.txt'
TEST_SUB_DATASETS = ('UPT_subset1_256_192', 'UPT_subset2_256_192')                              # dataset.py:1009
TEST_PAIR_LIST = 'test_pairs_front_list_shuffle_0508.txt'
SUB_DATASETS_512 = ('Zalando_512_320', 'Zalora_512_320', 'Deepfashion_512_320', 'MPV_512_320')     # dataset.py:1542
CHANGE_REGIONS = ('fullbody', 'upperbody', 'lowerbody')                                         # dataset.py:1679-1692

#----------------------------------------------------------------------------

class Dataset(torch.utils.data.Dataset):
    """The reference's base class (dataset.py:54-185) without its unused label machinery."""

    def __init__(self, name, raw_shape, max_size=None, use_labels=False, xflip=False, random_seed=0):
        if xflip:
            raise ValueError('xflip=True is not supported: no caller of the reference sets it, and its flip of the prepared tuple is undefined')
        self._name = name
        self._raw_shape = list(raw_shape)
        self._use_labels = use_labels
        self._raw_idx = np.arange(self._raw_shape[0], dtype=np.int64)
        if (max_size is not None) and (self._raw_idx.size > max_size):
            np.random.RandomState(random_seed).shuffle(self._raw_idx)
            self._raw_idx = np.sort(self._raw_idx[:max_size])
        self._xflip = np.zeros(self._raw_idx.size, dtype=np.uint8)

    def close(self):
        pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self._raw_idx.size

    @property
    def name(self):
        return self._name

    @property
    def image_shape(self):
        return list(self._raw_shape[1:])

    @property
    def num_channels(self):
        assert len(self.image_shape) == 3  # CHW
        return self.image_shape[0]

    @property
    def resolution(self):
        assert len(self.image_shape) == 3  # CHW
        assert self.image_shape[1] == self.image_shape[2]
        return self.image_shape[1]

    @property
    def vis_index(self):
        return self._vis_index

#----------------------------------------------------------------------------

def read_channel0(path):
    """Channel 0 of ``cv2.imread(path)`` (BGR): the blue component, which for a palette image is that of the palette colour,
    not the index; for a grayscale file the value itself."""
    with PIL.Image.open(path) as img:
        if img.mode == 'L':
            return np.array(img)
        return np.ascontiguousarray(np.array(img.convert('RGB'))[..., 2])


def read_keypoints(path):
    """``people[0].pose_keypoints_2d`` as float64 [18, 3], zeros when ``people`` is empty (dataset.py:738-746)."""
    with open(path, 'r') as f:
        data = json.load(f)
    if len(data['people']) == 0:
        return np.zeros((18, 3))
    return np.array(data['people'][0]['pose_keypoints_2d'], dtype=np.float64).reshape(-1, 3)


def fit_options(dataset, fit, fit_filter):
    """``fit`` (None, 'pad' or 'crop') and ``fit_filter`` ('bilinear' or 'box') of a data set, checked and kept as its attributes
    (this project's own: people of any size, fitted to the class's ``canvas`` per batch on the GPU by
    ``training.tryon_batch.fit_batch``; include/pasta_hip.h has the rule).  A ValueError names an unknown value."""
    from training.tryon_batch import FIT_MODES, fit_check
    fit_check(FIT_MODES[0] if fit is None else fit, fit_filter)
    dataset.fit, dataset.fit_filter = fit, fit_filter


def fit_sample(dataset, fname, shape):
    """The ``fit`` entry of a raw sample of a data set opened with ``fit``, after the rule's limits are checked for the file's
    ``shape``: an IOError names the file."""
    from training.tryon_batch import fit_limits, fit_rectangle
    H, W = dataset.canvas
    Hc, Wc, _, _ = fit_rectangle(shape[0], shape[1], H, W, dataset.fit)
    wrong = fit_limits(shape[0], shape[1], Hc, Wc)
    if wrong is not None:
        raise IOError('%s: cannot be fitted (%s) to %d x %d: %s' % (fname, dataset.fit, H, W, wrong))
    return dict(mode=dataset.fit, filter=dataset.fit_filter, canvas=(int(H), int(W)))


def pack_people(people):
    """[(image uint8 [h, w, 3], parsing uint8 [h, w]), ...] of any sizes -> (the photographs' bytes in one flat uint8 tensor, the
    label maps' in another, ``image_hw`` int32 [N, 2], ``image_offsets`` int64 [N]: each item's first PIXEL in both)."""
    hw = np.array([p[1].shape for p in people], np.int64).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum(hw[:, 0] * hw[:, 1])[:-1]]).astype(np.int64)
    image = np.concatenate([np.ascontiguousarray(p[0]).reshape(-1) for p in people])
    parsing = np.concatenate([np.ascontiguousarray(p[1]).reshape(-1) for p in people])
    return torch.from_numpy(image), torch.from_numpy(parsing), torch.from_numpy(hw.astype(np.int32)), torch.from_numpy(offsets)


ERASE_MASKS = ('files', 'none', 'strokes')          # UvitonDatasetFull(erase_masks=): where a training item's erase mask comes from


class UvitonDatasetFull(Dataset):
    """dataset.py:426-995 -- file lists, ``_vis_index`` and the ACGPN erase masks of a directory tree; ``__getitem__``
    returns the raw sample (see the module docstring): a dict with
    ``image`` uint8 [H, W, 3], ``parsing`` uint8 [H, W] (channel 0 as cv2.imread reads it), ``keypoints`` float64 [18, 3],
    ``erase_mask`` uint8 [h, w] (channel 0 of the ACGPN mask file ``raw_idx % count``, whatever its size) and ``raw_idx``.
    Key points stay float64 because the reference truncates and offsets them in float64.

    ``mirror_people=True`` (this project's own; the reference's ``xflip`` flips the prepared tuple, which is undefined here and stays
    refused) doubles the set: positions N .. 2N-1 are the people of positions 0 .. N-1 again, with ``xflip`` = 1 in the raw
    sample.  The files are read as they are: the builder mirrors the flagged items of a batch on the GPU
    (``training.tryon_batch.mirror_batch``; include/pasta_hip.h has the rule).  Without the option a sample has no ``xflip``.

    ``erase_masks`` (this project's own): ``'files'`` reads the ACGPN masks as above; ``'none'`` and ``'strokes'`` never look at
    ``train_random_mask_acgpn``, so a tree without it opens, and every ``erase_mask`` is a 1 x 1 zero, which erases nothing.  With
    ``'strokes'`` whoever numbers the batches attaches ``erase_strokes`` (the checked specification of
    ``training.tryon_batch.strokes_spec``, an attribute here as ``erase_masks`` is) and the builder draws a mask per item on the
    GPU (``training.tryon_batch.strokes_batch``; include/pasta_hip.h has the rule).

    ``fit`` = 'pad' or 'crop' with ``fit_filter`` = 'bilinear' or 'box' (this project's own): the photographs may have any size.
    The set is sized by the class's ``canvas`` instead of by file 0, ``content_width`` is the canvas width, ``resolution`` must be
    the canvas height, and a sample keeps its files' own size and carries ``fit`` (mode, filter, canvas): ``collate`` packs such
    samples and the builder fits them on the GPU (``training.tryon_batch.fit_batch``; include/pasta_hip.h has the rule).  A file
    outside the rule's limits raises IOError at load."""

    _sub_datasets = SUB_DATASETS
    canvas = (256, 192)
    _vis_sources = (('Zalando_256_192', 'image'), ('Deepfashion_256_192', os.path.join('image', 'train')))     # :461-472, in this order

    @staticmethod
    def _label_name(dataset, name):
        return name.replace('.jpg', '.png') if dataset == 'MPV_256_192' else name.replace('.jpg', '_label.png')

    def __init__(self, path, resolution=None, mirror_people=False, erase_masks='files', erase_strokes=None, fit=None, fit_filter='bilinear',
                 **super_kwargs):
        fit_options(self, fit, fit_filter)
        if erase_masks not in ERASE_MASKS:
            raise ValueError('erase_masks=%r is none of %s' % (erase_masks, ', '.join(ERASE_MASKS)))
        if erase_strokes is not None and erase_masks != 'strokes':
            raise ValueError("erase_strokes is a specification for erase_masks='strokes', not %r" % (erase_masks,))
        self.erase_masks = erase_masks
        self.erase_strokes = None
        if erase_masks == 'strokes':
            from training.tryon_batch import strokes_spec
            self.erase_strokes = strokes_spec(erase_strokes or {})
        self._path = path
        if not os.path.isdir(self._path):
            raise IOError('Path must point to a directory')
        self._type = 'dir'
        self._mirror_people = bool(mirror_people)
        self._image_fnames, self._kpt_fnames, self._parsing_fnames = [], [], []
        for dataset in self._sub_datasets:
            with open(os.path.join(self._path, dataset, PAIR_LIST), 'r') as f:
                for person in f.readlines():
                    if not person.strip():
                        continue
                    person = person.strip().split()[0]
                    self._image_fnames.append(os.path.join(dataset, 'image', person))
                    self._kpt_fnames.append(os.path.join(dataset, 'keypoints', person.replace('.jpg', '_keypoints.json')))
                    self._parsing_fnames.append(os.path.join(dataset, 'parsing', self._label_name(dataset, person)))

        vis_index = []
        for image_name in sorted(os.listdir(os.path.join(self._path, 'train_img_vis'))):         # :461-472
            for dataset, folder in self._vis_sources:
                if os.path.exists(os.path.join(self._path, dataset, folder, image_name)):
                    vis_index.append(self._image_fnames.index(os.path.join(dataset, folder, image_name)))
                    break
        self._vis_index = vis_index

        self._random_mask_acgpn_fnames = []
        if self.erase_masks == 'files':
            acgpn_dir = os.path.join(self._path, 'train_random_mask_acgpn')
            self._random_mask_acgpn_fnames = [os.path.join(acgpn_dir, name) for name in os.listdir(acgpn_dir)]     # os.listdir order (:476)
        self._mask_acgpn_numbers = len(self._random_mask_acgpn_fnames)

        PIL.Image.init()
        if len(self._image_fnames) == 0:
            raise IOError('No image files found in the specified path')
        h, w, c = self.canvas + (3,) if self.fit is not None else self._load_image(0).shape
        self.content_width = int(w)                            # the photographs' own width, which the batch builder pads to the square
        raw_shape = [len(self._image_fnames), c, h, h]         # the padded square, as the reference's image_shape
        if resolution is not None and (raw_shape[2] != resolution or raw_shape[3] != resolution):
            raise IOError('Image files do not match the specified resolution')
        super().__init__(name=os.path.splitext(os.path.basename(self._path))[0], raw_shape=raw_shape, **super_kwargs)
        if self._mirror_people:         # after max_size, as the reference's base class does with xflip (dataset.py:75-79)
            self._raw_idx = np.tile(self._raw_idx, 2)
            self._xflip = np.concatenate([self._xflip, np.ones_like(self._xflip)])

    def _load_image(self, raw_idx):
        image = np.array(PIL.Image.open(os.path.join(self._path, self._image_fnames[raw_idx])))
        if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < image.shape[1]:
            raise IOError('%s: expected an RGB image at least as tall as wide, got %s' % (self._image_fnames[raw_idx], image.shape))
        return image

    def _fit_sample(self, raw_idx, sample):
        if self.fit is not None:
            sample['fit'] = fit_sample(self, self._image_fnames[raw_idx], sample['image'].shape)
        return sample

    def load_raw(self, raw_idx):
        image = self._load_image(raw_idx)
        parsing = read_channel0(os.path.join(self._path, self._parsing_fnames[raw_idx]))
        if parsing.shape != image.shape[:2]:
            raise IOError('%s: label map %s does not match the image %s' % (self._parsing_fnames[raw_idx], parsing.shape, image.shape[:2]))
        keypoints = read_keypoints(os.path.join(self._path, self._kpt_fnames[raw_idx]))
        if self.erase_masks == 'files':
            erase = read_channel0(self._random_mask_acgpn_fnames[raw_idx % self._mask_acgpn_numbers])
        else:
            erase = np.zeros([1, 1], np.uint8)
        return self._fit_sample(raw_idx, dict(image=image, parsing=parsing, keypoints=keypoints, erase_mask=erase, raw_idx=int(raw_idx)))

    def __getitem__(self, idx):
        sample = self.load_raw(self._raw_idx[idx])
        if self._mirror_people:
            sample['xflip'] = int(self._xflip[idx])
        return sample


class UvitonDatasetFull_512(UvitonDatasetFull):
    """The training layout at 512 x 320 (this project's own; the reference ships only the 512 x 320 test set):
    ``Zalando_512_320``, ``Zalora_512_320``, ``Deepfashion_512_320`` and ``MPV_512_320``, in this order, each with ``image/``,
    ``keypoints/``, ``parsing/`` and the training list of ``UvitonDatasetFull``; label maps are ``parsing/<stem>_label.png`` in
    all four, as in ``UvitonDatasetFull_512_test``; ``train_img_vis/`` names people of ``Zalando_512_320/image`` or
    ``Deepfashion_512_320/image/train``.  Raw samples as ``UvitonDatasetFull``'s, so ``collate`` serves both."""

    _sub_datasets = SUB_DATASETS_512
    canvas = (512, 320)
    _vis_sources = (('Zalando_512_320', 'image'), ('Deepfashion_512_320', os.path.join('image', 'train')))

    @staticmethod
    def _label_name(dataset, name):
        return name.replace('.jpg', '_label.png')


def training_set_class(path):
    """The class name of the training data set a tree holds: the 512 x 320 one when ``Zalando_512_320`` is present and
    ``Zalando_256_192`` is not, else the 256 x 192 one (also for a tree with neither, whose error names the 256 layout)."""
    is_512 = os.path.isdir(os.path.join(path, SUB_DATASETS_512[0])) and not os.path.isdir(os.path.join(path, SUB_DATASETS[0]))
    return 'training.dataset.UvitonDatasetFull_512' if is_512 else 'training.dataset.UvitonDatasetFull'

#----------------------------------------------------------------------------

def collate(samples):
    """A list of raw samples -> one batch: ``image`` uint8 [N, H, W, 3], ``parsing`` uint8 [N, H, W], ``keypoints`` float64
    [N, 18, 3], ``erase_masks`` uint8 [N, h_max, w_max] (each mask in the top-left corner) with ``erase_hw`` int32 [N, 2]
    (its own size), ``raw_idx`` int64 [N]; ``xflip`` uint8 [N] when the samples carry it (``mirror_people``).  Samples that carry
    ``fit`` (people of their own sizes) are PACKED instead of stacked (``pack_people``): ``image`` and ``parsing`` are flat, with
    ``image_hw`` int32 [N, 2] and ``image_offsets`` int64 [N] next to them and the samples' ``fit``.  Use as the DataLoader's
    ``collate_fn``."""
    n = len(samples)
    h_max = max(s['erase_mask'].shape[0] for s in samples)
    w_max = max(s['erase_mask'].shape[1] for s in samples)
    erase = np.zeros([n, h_max, w_max], np.uint8)
    erase_hw = np.zeros([n, 2], np.int32)
    for i, s in enumerate(samples):
        h, w = s['erase_mask'].shape
        erase[i, :h, :w] = s['erase_mask']
        erase_hw[i] = h, w
    if 'fit' in samples[0]:
        image, parsing, image_hw, image_offsets = pack_people([(s['image'], s['parsing']) for s in samples])
        people = dict(image=image, parsing=parsing, image_hw=image_hw, image_offsets=image_offsets, fit=dict(samples[0]['fit']))
    else:
        people = dict(image=torch.from_numpy(np.stack([s['image'] for s in samples])),
                      parsing=torch.from_numpy(np.stack([s['parsing'] for s in samples])))
    batch = dict(people, keypoints=torch.from_numpy(np.stack([s['keypoints'] for s in samples])),
                 erase_masks=torch.from_numpy(erase), erase_hw=torch.from_numpy(erase_hw),
                 raw_idx=torch.as_tensor([s['raw_idx'] for s in samples], dtype=torch.int64))
    if 'xflip' in samples[0]:
        batch['xflip'] = torch.as_tensor([s['xflip'] for s in samples], dtype=torch.uint8)
    return batch

#----------------------------------------------------------------------------

class _SubDatasetCanvas:
    """The ``canvas`` class attribute of the test sets, which differ in ``_sub_datasets`` and ``_label_name`` only: the canvas of the
    folders a class reads."""

    def __get__(self, obj, owner):
        return (512, 320) if owner._sub_datasets is SUB_DATASETS_512 else (256, 192)


class UvitonDatasetV19_test(Dataset):
    """dataset.py:997-1153 -- the unpaired test pairs of ``UPT_subset1_256_192`` and ``UPT_subset2_256_192``: each line
    ``person clothes`` of ``test_pairs_front_list_shuffle_0508.txt``, in file order.  ``__getitem__`` returns the raw pair (see
    the module docstring): a dict with the person's ``image`` uint8 [H, W, 3], ``parsing`` uint8 [H, W] (channel 0 as
    cv2.imread reads it) and ``keypoints`` float64 [18, 3] (unshifted), the same three of the clothes donor as
    ``clothes_image`` / ``clothes_parsing`` / ``clothes_keypoints``, and ``person_name`` / ``clothes_name`` (the reference's
    relative paths, ``<sub-dataset>/image/<file>``)."""

    _sub_datasets = TEST_SUB_DATASETS
    canvas = _SubDatasetCanvas()                # (256, 192), or (512, 320) in the classes that read the ``*_512_320`` folders
    fit, fit_filter = None, 'bilinear'          # every test set takes them as UvitonDatasetFull does (``fit_options``)

    @staticmethod
    def _label_name(dataset, name):
        return name.replace('.jpg', '.png') if dataset == 'MPV_256_192' else name.replace('.jpg', '_label.png')     # :1030-1033

    def _open_tree(self, path):
        self._path = path
        if not os.path.isdir(self._path):
            raise IOError('Path must point to a directory')
        self._type = 'dir'

    def _init_items(self, first_person, count, resolution, super_kwargs, nothing='No image files found in the specified path'):
        """The end of every test set's __init__: ``count`` items, sized by the files ``first_person`` (image, parsing, key points)."""
        self._vis_index = list(range(64))
        PIL.Image.init()
        if count == 0:
            raise IOError(nothing)
        h, w, c = self.canvas + (3,) if self.fit is not None else self._load_person(*first_person)[0].shape
        raw_shape = [count, c, h, h]                           # the padded square, as the reference's image_shape
        if resolution is not None and (raw_shape[2] != resolution or raw_shape[3] != resolution):
            raise IOError('Image files do not match the specified resolution')
        Dataset.__init__(self, name=os.path.splitext(os.path.basename(self._path))[0], raw_shape=raw_shape, **super_kwargs)

    def __init__(self, path, resolution=None, fit=None, fit_filter='bilinear', **super_kwargs):
        fit_options(self, fit, fit_filter)
        self._open_tree(path)
        self._image_fnames, self._kpt_fnames, self._parsing_fnames = [], [], []
        self._clothes_image_fnames, self._clothes_kpt_fnames, self._clothes_parsing_fnames = [], [], []
        for dataset in self._sub_datasets:
            with open(os.path.join(self._path, dataset, TEST_PAIR_LIST), 'r') as f:
                for line in f.readlines():
                    if not line.strip():
                        continue
                    person, clothes = line.strip().split()
                    for name, images, kpts, labels in ((person, self._image_fnames, self._kpt_fnames, self._parsing_fnames),
                                                       (clothes, self._clothes_image_fnames, self._clothes_kpt_fnames, self._clothes_parsing_fnames)):
                        images.append(os.path.join(dataset, 'image', name))
                        kpts.append(os.path.join(dataset, 'keypoints', name.replace('.jpg', '_keypoints.json')))
                        labels.append(os.path.join(dataset, 'parsing', self._label_name(dataset, name)))
        first = [names[0] for names in (self._image_fnames, self._parsing_fnames, self._kpt_fnames) if names]
        self._init_items(first, len(self._image_fnames), resolution, super_kwargs)

    def _load_person(self, image_fname, parsing_fname, kpt_fname):
        image = np.array(PIL.Image.open(os.path.join(self._path, image_fname)))
        if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < image.shape[1]:
            raise IOError('%s: expected an RGB image at least as tall as wide, got %s' % (image_fname, image.shape))
        parsing = read_channel0(os.path.join(self._path, parsing_fname))
        if parsing.shape != image.shape[:2]:
            raise IOError('%s: label map %s does not match the image %s' % (parsing_fname, parsing.shape, image.shape[:2]))
        if self.fit is not None:
            fit_sample(self, image_fname, image.shape)              # the limits, at load
        return image, parsing, read_keypoints(os.path.join(self._path, kpt_fname))

    def _fit_entry(self, sample):
        if self.fit is not None:
            sample['fit'] = dict(mode=self.fit, filter=self.fit_filter, canvas=tuple(int(v) for v in self.canvas))
        return sample

    def load_raw(self, raw_idx):
        image, parsing, keypoints = self._load_person(self._image_fnames[raw_idx], self._parsing_fnames[raw_idx], self._kpt_fnames[raw_idx])
        c_image, c_parsing, c_keypoints = self._load_person(self._clothes_image_fnames[raw_idx], self._clothes_parsing_fnames[raw_idx],
                                                            self._clothes_kpt_fnames[raw_idx])
        if self.fit is None and c_image.shape != image.shape:
            raise IOError('%s: the clothes image %s does not match the person %s' % (self._clothes_image_fnames[raw_idx], c_image.shape, image.shape))
        return self._fit_entry(dict(image=image, parsing=parsing, keypoints=keypoints, clothes_image=c_image, clothes_parsing=c_parsing,
                                    clothes_keypoints=c_keypoints, person_name=self._image_fnames[raw_idx],
                                    clothes_name=self._clothes_image_fnames[raw_idx], raw_idx=int(raw_idx)))

    def __getitem__(self, idx):
        return self.load_raw(self._raw_idx[idx])


class UvitonDatasetFull_512_test(UvitonDatasetV19_test):
    """dataset.py:1528-2214 -- the unpaired test pairs at 512 x 320 of ``Zalando_512_320``, ``Zalora_512_320``,
    ``Deepfashion_512_320`` and ``MPV_512_320``, in this order: each line ``person clothes`` of their
    ``test_pairs_front_list_shuffle_0508.txt``, in file order.  Label maps are ``parsing/<stem>_label.png`` in all four (the
    256 set's ``.png`` exception for MPV does not apply, :1562-1563).  ``change_region`` is 'fullbody', 'upperbody' or
    'lowerbody': which garments the person takes from the donor.

    Differences from the reference, by design: ``__getitem__`` returns the raw pair, with the keys of
    ``UvitonDatasetV19_test`` (so ``collate_pairs`` serves both), and not the prepared 12-tuple: stick figure, palm and label
    masks, the region's warps and composites and the float conversions run for a whole batch on the GPU in
    ``training.tryon_regions.TryOnRegionBatchBuilder``, which takes ``change_region`` itself.  Key points stay float64 and
    unshifted.  An unknown ``change_region`` raises ValueError here, at construction; the reference raises it at the first
    item (:1692)."""
    _sub_datasets = SUB_DATASETS_512

    @staticmethod
    def _label_name(dataset, name):
        return name.replace('.jpg', '_label.png')

    def __init__(self, path, change_region, resolution=None, **super_kwargs):
        if change_region not in CHANGE_REGIONS:
            raise ValueError('change region %s is invalid.' % change_region)
        self._change_region = change_region
        super().__init__(path, resolution=resolution, **super_kwargs)

    @property
    def change_region(self):
        return self._change_region


def collate_pairs(samples):
    """A list of raw pairs -> one batch: ``image`` / ``clothes_image`` uint8 [N, H, W, 3], ``parsing`` / ``clothes_parsing``
    uint8 [N, H, W], ``keypoints`` / ``clothes_keypoints`` float64 [N, 18, 3], ``person_name`` / ``clothes_name`` lists of str,
    ``raw_idx`` int64 [N].  Use as the DataLoader's ``collate_fn``."""
    stack = lambda key: torch.from_numpy(np.stack([s[key] for s in samples]))
    out = {k: stack(k) for k in ('image', 'parsing', 'keypoints', 'clothes_image', 'clothes_parsing', 'clothes_keypoints')}
    out.update(person_name=[s['person_name'] for s in samples], clothes_name=[s['clothes_name'] for s in samples],
               raw_idx=torch.as_tensor([s['raw_idx'] for s in samples], dtype=torch.int64))
    return out


class UvitonOutfits_512_test(UvitonDatasetV19_test):
    """This project's own: outfits at 512 x 320, a person with the upper garment of one donor and the lower garment of another.
    ``outfits_file`` is a text file of lines ``person upper lower`` (blank lines skipped), each name ``<sub-dataset>/<file>.jpg``
    with the sub-dataset one of ``SUB_DATASETS_512``, resolved as ``UvitonDatasetFull_512_test`` resolves a pair-list name
    (``<sub>/image/<file>``, ``<sub>/keypoints/<stem>_keypoints.json``, ``<sub>/parsing/<stem>_label.png``); the three may come
    from different sub-datasets.  ``upper`` or ``lower`` may be ``-``: the person keeps that garment of their own (``- -`` is the
    self-pair the 512 model is trained on).  The pair lists are not read.  A line without exactly three fields, an unknown
    sub-dataset or ``-`` as the person raises ValueError with the file and the 1-based line number; a missing file raises IOError
    at load.  The change regions are three of its cases: full body (P, D, D), upper body (P, D, -), lower body (P, -, D).

    ``__getitem__`` returns the raw outfit: the person's ``image`` / ``parsing`` / ``keypoints`` (as the pairs' data set),
    the same three as ``upper_*`` and ``lower_*``, ``person_name`` / ``upper_name`` / ``lower_name`` (``<sub>/image/<file>``)
    and ``raw_idx``, the line's position among the outfits.  For ``-`` the names and arrays are the person's own; a file named
    twice on a line is decoded once.  ``collate_outfits`` makes the batch ``training.tryon_regions.TryOnOutfitBatchBuilder``
    takes."""

    _sub_datasets = SUB_DATASETS_512
    _label_name = staticmethod(UvitonDatasetFull_512_test._label_name)

    def __init__(self, path, outfits_file, resolution=None, fit=None, fit_filter='bilinear', **super_kwargs):
        fit_options(self, fit, fit_filter)
        self._open_tree(path)
        self._outfits = []              # per line: the (image, parsing, keypoints) file names of person, upper, lower
        with open(outfits_file, 'r') as f:
            for number, line in enumerate(f.readlines(), 1):
                if not line.strip():
                    continue
                where = '%s, line %d' % (outfits_file, number)
                fields = line.split()
                if len(fields) != 3:
                    raise ValueError('%s: expected "person upper lower", got %d fields' % (where, len(fields)))
                if fields[0] == '-':
                    raise ValueError('%s: the person cannot be "-"' % where)
                people = []
                for name in fields:
                    if name == '-':
                        people.append(people[0])
                        continue
                    dataset, _, fname = name.partition('/')
                    if dataset not in self._sub_datasets or not fname:
                        raise ValueError('%s: %r is not <sub-dataset>/<file>.jpg with the sub-dataset one of %s'
                                         % (where, name, ', '.join(self._sub_datasets)))
                    people.append((os.path.join(dataset, 'image', fname), os.path.join(dataset, 'parsing', self._label_name(dataset, fname)),
                                   os.path.join(dataset, 'keypoints', fname.replace('.jpg', '_keypoints.json'))))
                self._outfits.append(tuple(people))
        self._init_items(self._outfits[0][0] if self._outfits else None, len(self._outfits), resolution, super_kwargs,
                         'No outfits found in %s' % outfits_file)

    def load_raw(self, raw_idx):
        outfit = self._outfits[raw_idx]
        decoded, out = {}, dict(raw_idx=int(raw_idx))
        for role, prefix, files in zip(('person', 'upper', 'lower'), ('', 'upper_', 'lower_'), outfit):
            if files not in decoded:
                decoded[files] = self._load_person(*files)
            image, parsing, keypoints = decoded[files]
            if self.fit is None and image.shape != decoded[outfit[0]][0].shape:
                raise IOError('%s: the image %s does not match the person %s' % (files[0], image.shape, decoded[outfit[0]][0].shape))
            out.update({prefix + 'image': image, prefix + 'parsing': parsing, prefix + 'keypoints': keypoints, role + '_name': files[0]})
        return self._fit_entry(out)


class UvitonOutfits_256_test(UvitonOutfits_512_test):
    """This project's own: outfits for the 256 x 192 model, ``UvitonOutfits_512_test`` on the 256 test tree.  The sub-dataset of
    a name is one of ``TEST_SUB_DATASETS`` and label maps follow ``UvitonDatasetV19_test``'s rule (``parsing/<stem>_label.png``;
    ``parsing/<stem>.png`` for ``MPV_256_192``).  The line format, the ``-`` rule, the errors and the raw outfit are the 512
    class's, so ``collate_outfits`` serves both; ``training.tryon_pairs.TryOnPairOutfitBatchBuilder`` takes its batches.  The
    change regions are three of its cases: upper body (P, D, -), what test.py does with a pair, lower body (P, -, D) and full
    body (P, D, D)."""

    _sub_datasets = TEST_SUB_DATASETS
    _label_name = staticmethod(UvitonDatasetV19_test._label_name)


def collate_outfits(samples):
    """A list of raw outfits -> one batch in which every DISTINCT person (by name) is stacked once, in the order of first
    appearance (samples in order; person, upper, lower within a sample): ``people_image`` uint8 [M, H, W, 3], ``people_parsing``
    uint8 [M, H, W], ``people_keypoints`` float64 [M, 18, 3], ``people_name`` list of str; ``person_idx`` / ``upper_idx`` /
    ``lower_idx`` int64 [N] into that stack; ``person_name`` / ``upper_name`` / ``lower_name`` lists of str, ``raw_idx`` int64
    [N].  A person who keeps a garment, or a donor several outfits of the batch use, is uploaded and solved for once.  Samples that
    carry ``fit`` (people of their own sizes) are PACKED instead of stacked, as ``collate`` packs them: ``people_image`` and
    ``people_parsing`` flat, with ``people_image_hw`` int32 [M, 2], ``people_image_offsets`` int64 [M] and ``fit``.  Use as the
    DataLoader's ``collate_fn``."""
    roles = (('person', ''), ('upper', 'upper_'), ('lower', 'lower_'))
    slot, people = {}, []
    index = {role: [] for role, _ in roles}
    for s in samples:
        for role, prefix in roles:
            name = s[role + '_name']
            if name not in slot:
                slot[name] = len(people)
                people.append((s[prefix + 'image'], s[prefix + 'parsing'], s[prefix + 'keypoints']))
            index[role].append(slot[name])
    if 'fit' in samples[0]:
        image, parsing, image_hw, image_offsets = pack_people([p[:2] for p in people])
        out = dict(people_image=image, people_parsing=parsing, people_image_hw=image_hw, people_image_offsets=image_offsets,
                   people_keypoints=torch.from_numpy(np.stack([p[2] for p in people])), fit=dict(samples[0]['fit']))
    else:
        out = {key: torch.from_numpy(np.stack([p[k] for p in people])) for k, key in enumerate(('people_image', 'people_parsing', 'people_keypoints'))}
    out['people_name'] = list(slot)
    for role, _ in roles:
        out[role + '_idx'] = torch.as_tensor(index[role], dtype=torch.int64)
        out[role + '_name'] = [s[role + '_name'] for s in samples]
    out['raw_idx'] = torch.as_tensor([s['raw_idx'] for s in samples], dtype=torch.int64)
    return out


def pair_as_outfit(sample, change_region):
    """A raw pair (``UvitonDatasetV19_test``) -> the raw outfit of a change region: upper body (P, D, P), the pair as test.py
    dresses it, lower body (P, P, D), full body (P, D, D).  ``clothes_name`` stays."""
    if change_region not in CHANGE_REGIONS:
        raise ValueError('change region %s is invalid.' % change_region)
    out = {k: sample[k] for k in ('image', 'parsing', 'keypoints', 'person_name', 'clothes_name', 'raw_idx') + (('fit',) if 'fit' in sample else ())}
    for role, prefix, donor in (('upper', 'upper_', change_region != 'lowerbody'), ('lower', 'lower_', change_region != 'upperbody')):
        src, name = ('clothes_', 'clothes_name') if donor else ('', 'person_name')
        out.update({prefix + k: sample[src + k] for k in ('image', 'parsing', 'keypoints')})
        out[role + '_name'] = sample[name]
    return out


def collate_region_outfits(change_region, samples):
    """``collate_outfits`` of raw PAIRS taken as the outfits of ``change_region`` (``pair_as_outfit``), with the pairs'
    ``clothes_name``.  ``functools.partial(collate_region_outfits, region)`` is the DataLoader's ``collate_fn``."""
    out = collate_outfits([pair_as_outfit(s, change_region) for s in samples])
    out['clothes_name'] = [s['clothes_name'] for s in samples]
    return out


def pairs_batch_as_outfits(raw, change_region):
    """A COLLATED batch of pairs (``collate_pairs``) -> the batch ``collate_outfits`` makes of the same pairs taken as the outfits
    of ``change_region``, without looking for people named twice: the stack is the N persons followed by the N clothes donors
    (M = 2N, ``people_name`` may repeat), ``person_idx`` 0..N-1, ``upper_idx`` / ``lower_idx`` the donors' N..2N-1 where the region
    takes that garment from the donor.  ``clothes_name`` stays.  The tensors are concatenated where they are: a batch whose
    images a builder has uploaded is stacked on the device.  The pair builders are the outfit builders behind this function; the
    command lines go through ``collate_region_outfits`` in the loader's workers instead, which does deduplicate."""
    if change_region not in CHANGE_REGIONS:
        raise ValueError('change region %s is invalid.' % change_region)
    out = {'people_' + k: torch.cat([torch.as_tensor(raw[k]), torch.as_tensor(raw['clothes_' + k])]) for k in ('image', 'parsing', 'keypoints')}
    person = torch.arange(len(raw['person_name']), dtype=torch.int64)
    index = dict(person=person, clothes=person + len(person))
    names = dict(person=list(raw['person_name']), clothes=list(raw['clothes_name']))
    out.update(people_name=names['person'] + names['clothes'], person_idx=person, person_name=names['person'], clothes_name=names['clothes'],
               raw_idx=raw['raw_idx'])
    for role, donor in (('upper', change_region != 'lowerbody'), ('lower', change_region != 'upperbody')):
        out[role + '_idx'], out[role + '_name'] = index['clothes' if donor else 'person'], names['clothes' if donor else 'person']
    return out

#----------------------------------------------------------------------------
