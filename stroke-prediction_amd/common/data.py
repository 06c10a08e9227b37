"""Batch-dict contract and sample transforms of the reference data layer (``common/data.py``), on the GPU.

The NIfTI dataset itself stays out of scope (private data, nibabel); what is mirrored here is what sits between a
loaded sample and the network (SURVEY.md 8 "next" row N4): the transform classes of ``common/data.py:215-351`` with the
same names, constructor arguments and sample-dict semantics, operating on **device tensors**.  A sample is the
reference's dict -- ``images`` / ``labels`` as ``(x, y, z, c)`` arrays, ``clinical`` -- whose arrays are
``torch.cuda`` fp32 tensors (``to_device(sample)`` uploads a numpy sample once); every transform returns device
tensors, so a pipeline ``Compose([HemisphericFlip(), ElasticDeform(), ToTensor()])`` never leaves the GPU.  Flip,
patch, pad and the layout permutation are index arithmetic (torch views + one copy); the elastic deformation runs on the
HIP kernels ``sp_gaussian_filter3d`` / ``sp_map_coordinates_linear`` (csrc/sp_transform.hip).  Random decisions come
from the same host generators as in the reference (``random`` / ``numpy.random.RandomState``), so a seeded pipeline
reproduces the reference's augmentation; ``ElasticDeform(device_noise=True)`` draws the noise on the device instead.
``BatchElasticDeform`` is the batch-level form: flip + elastic deformation of a whole collated batch in five launches
(csrc/sp_augment.hip), handed to the loader factories as ``batch_transform``.  ``device_cache=True`` on the factories keeps
every case on the device (``DeviceCaseCache``) and builds each batch -- flip, padding, patch, layout, stack -- with one launch of
``sp_patch_gather_batch`` (csrc/sp_gather.hip; ``CachedBatchLoader``).  ``PatchAugment`` (``patch_augment=`` on the factories) makes
that launch ``sp_patch_sample_batch`` (csrc/sp_sample.hip): rotation, scaling, elastic deformation and an intensity change per
sample, images and labels through one field, in the kernel that builds the batch.  ``ForegroundOversample`` (``foreground=``) forces
a share of each cached batch onto lesion: ``sp_patch_origins_fg`` (csrc/sp_fgpatch.hip) rewrites those samples' origins on the device.
``IntensityAugment`` is a second ``batch_transform``: blur, noise, brightness, contrast and gamma of the images of a batch that already
sits on the device, in two launches (five with blur; csrc/sp_intensity.hip).
"""
import datetime
import random

import numpy as np
import torch

KEY_CASE_ID = 'case_id'
KEY_CLINICAL_IDX = 'clinical_idx'
KEY_IMAGES = 'images'
KEY_LABELS = 'labels'
KEY_GLOBAL = 'clinical'

DIM_HORIZONTAL_NUMPY_3D = 0
DIM_DEPTH_NUMPY_3D = 2
DIM_CHANNEL_NUMPY_3D = 3
DIM_CHANNEL_TORCH3D_5 = 1     # tensors are B x C x D x H x W


def _present(v):
    """The reference marks a missing entry with ``[]`` (data.py:102-105)."""
    if isinstance(v, torch.Tensor):
        return v.numel() > 0
    if isinstance(v, np.ndarray):
        return v.size > 0
    return False


def emptyCopyFromSample(sample):
    """data.py:102-105."""
    result = {KEY_CASE_ID: int(sample[KEY_CASE_ID]), KEY_CLINICAL_IDX: sample.get(KEY_CLINICAL_IDX, 0),
              KEY_IMAGES: [], KEY_LABELS: [], KEY_GLOBAL: []}
    return result


def to_device(sample, device="cuda"):
    """Upload the arrays of a numpy sample (fp32) -- the one host-to-device copy of the pipeline."""
    out = dict(sample)
    for k in (KEY_IMAGES, KEY_LABELS, KEY_GLOBAL):
        v = sample.get(k, [])
        if isinstance(v, np.ndarray) and v.size:
            out[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(device)
    return out


def _require_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError("%s (stroke_prediction_amd) works on CUDA tensors; upload the sample with to_device() first" % what)


class HemisphericFlipFixedToCaseId(object):
    """Flip along the X axis for case ids above ``split_id`` (data.py:215-231)."""

    def __init__(self, split_id):
        self.split_id = split_id

    def __call__(self, sample):
        if int(sample[KEY_CASE_ID]) > self.split_id:
            return _flip(sample)
        return sample


class HemisphericFlip(object):
    """Flip along the X axis with probability 1/2 (data.py:234-246; ``random.random()`` like the reference)."""

    def __call__(self, sample):
        if random.random() > 0.5:
            return _flip(sample)
        return sample


def _flip(sample):
    result = emptyCopyFromSample(sample)
    for k in (KEY_IMAGES, KEY_LABELS, KEY_GLOBAL):
        if _present(sample[k]):
            _require_cuda(sample[k], "HemisphericFlip")
            result[k] = torch.flip(sample[k], (DIM_HORIZONTAL_NUMPY_3D,))
    return result


class RandomPatch(object):
    """Random patches of a certain size; labels cropped by the network's padding (data.py:249-277)."""

    def __init__(self, w, h, d, pad_x, pad_y, pad_z):
        self._padx, self._pady, self._padz = pad_x, pad_y, pad_z
        self._w, self._h, self._d = w, h, d

    def __call__(self, sample):
        sx, sy, sz, _ = sample[KEY_IMAGES].shape
        rand_x = random.randint(0, sx - self._w)
        rand_y = random.randint(0, sy - self._h)
        rand_z = random.randint(0, sz - self._d)
        result = emptyCopyFromSample(sample)
        if _present(sample[KEY_IMAGES]):
            result[KEY_IMAGES] = sample[KEY_IMAGES][rand_x: rand_x + self._w, rand_y: rand_y + self._h,
                                                    rand_z: rand_z + self._d, :]
        if _present(sample[KEY_LABELS]):
            result[KEY_LABELS] = sample[KEY_LABELS][rand_x: rand_x + self._w - 2 * self._padx,
                                                    rand_y: rand_y + self._h - 2 * self._pady,
                                                    rand_z: rand_z + self._d - 2 * self._padz, :]
        result[KEY_GLOBAL] = sample[KEY_GLOBAL]
        return result


class PadImages(object):
    """Pad images with a constant in all 6 directions (data.py:280-296)."""

    def __init__(self, pad_x, pad_y, pad_z, pad_value=0):
        self._padx, self._pady, self._padz = pad_x, pad_y, pad_z
        self._pad_value = float(pad_value)

    def __call__(self, sample):
        result = emptyCopyFromSample(sample)
        if _present(sample[KEY_IMAGES]):
            img = sample[KEY_IMAGES]
            _require_cuda(img, "PadImages")
            sx, sy, sz, sc = img.shape
            out = torch.full((sx + 2 * self._padx, sy + 2 * self._pady, sz + 2 * self._padz, sc), self._pad_value,
                             dtype=torch.float32, device=img.device)
            out[self._padx:sx + self._padx, self._pady:sy + self._pady, self._padz:sz + self._padz, :] = img
            result[KEY_IMAGES] = out
        result[KEY_LABELS] = sample[KEY_LABELS]
        result[KEY_GLOBAL] = sample[KEY_GLOBAL]
        return result


class ToTensor(object):
    """(x, y, z, c) -> (c, z, y, x) (data.py:299-310); the arrays already are tensors here, the permutation is a view."""

    def __call__(self, sample):
        result = emptyCopyFromSample(sample)
        for k in (KEY_IMAGES, KEY_LABELS, KEY_GLOBAL):
            if _present(sample[k]):
                v = sample[k] if isinstance(sample[k], torch.Tensor) else torch.from_numpy(sample[k])
                result[k] = v.permute(3, 2, 1, 0)
        return result


class ElasticDeform(object):
    """Elastic deformation [Simard2003] of the label (and optionally image) channels (data.py:313-351): three
    Gaussian-smoothed uniform noise fields scaled by alpha (the third by 0.22 * alpha) displace the sampling grid,
    first-order interpolation, zero outside.  Noise: ``random_state.rand`` on the host exactly like the reference (one
    5.5 MB upload per channel at 128 x 128 x 28), or ``device_noise=True``: torch's device generator."""

    def __init__(self, alpha=100, sigma=4, apply_to_images=False, device_noise=False):
        self._alpha = alpha
        self._sigma = sigma
        self._apply_to_images = apply_to_images
        self._device_noise = device_noise

    def _smoothed_noise(self, shape, sigma, random_state, device, tmp):
        from stroke_prediction_amd.runtime import lib as L, ops as O
        if self._device_noise:
            noise = torch.rand(shape, dtype=torch.float32, device=device) * 2 - 1
        else:
            noise = torch.from_numpy((random_state.rand(*shape) * 2 - 1).astype(np.float32)).to(device)
        field = torch.empty_like(noise)
        L.call("sp_gaussian_filter3d", O.ptr(noise), O.ptr(field), O.ptr(tmp), shape[0], shape[1], shape[2], float(sigma), 4.0,
               O.stream())
        return field

    def elastic_transform(self, image, alpha=100, sigma=4, random_state=None):
        from stroke_prediction_amd.runtime import lib as L, ops as O
        _require_cuda(image, "ElasticDeform")
        new_seed = datetime.datetime.now().second + datetime.datetime.now().microsecond
        if random_state is None:
            random_state = np.random.RandomState(new_seed)
        shape = tuple(image.shape)
        if len(shape) != 3 or shape[0] != shape[1]:
            # the reference adds meshgrid(indexing='xy') grids of shape (s1, s0, s2) to fields of shape (s0, s1, s2)
            raise ValueError("elastic_transform needs a (n, n, d) volume (data.py:336-337), got %r" % (shape,))
        img = image.contiguous().float()
        tmp = torch.empty_like(img)
        dx = self._smoothed_noise(shape, sigma, random_state, img.device, tmp)
        dy = self._smoothed_noise(shape, sigma, random_state, img.device, tmp)
        dz = self._smoothed_noise(shape, sigma, random_state, img.device, tmp)
        out = torch.empty_like(img)
        # indices = (y + dy, x + dx, z + dz) with x, y, z = meshgrid(...) in 'xy' indexing: y is the axis-0 index and x
        # the axis-1 index -- axis 0 is displaced by the SECOND field, axis 1 by the first (data.py:336-337)
        L.call("sp_map_coordinates_linear", O.ptr(img), O.ptr(dy), O.ptr(dx), O.ptr(dz), float(alpha), float(alpha),
               float(alpha) * 0.22, 0.0, O.ptr(out), shape[0], shape[1], shape[2], O.stream())
        return out, random_state

    def __call__(self, sample):
        labels = sample[KEY_LABELS]
        _require_cuda(labels, "ElasticDeform")
        if not labels.is_contiguous():
            labels = sample[KEY_LABELS] = labels.contiguous()
        res, random_state = self.elastic_transform(labels[:, :, :, 0], self._alpha, self._sigma)
        labels[:, :, :, 0] = res
        for c in range(1, labels.shape[3]):
            labels[:, :, :, c], _ = self.elastic_transform(labels[:, :, :, c], self._alpha, self._sigma,
                                                           random_state=random_state)
        if self._apply_to_images and _present(sample[KEY_IMAGES]):
            images = sample[KEY_IMAGES]
            if not images.is_contiguous():
                images = sample[KEY_IMAGES] = images.contiguous()
            for c in range(images.shape[3]):
                images[:, :, :, c], _ = self.elastic_transform(images[:, :, :, c], self._alpha, self._sigma,
                                                               random_state=random_state)
        return sample


class BatchElasticDeform(object):
    """``HemisphericFlip`` / ``HemisphericFlipFixedToCaseId`` followed by ``ElasticDeform``, for a whole COLLATED batch: a
    callable on the batch dict (``labels`` (B, C, Z, Y, X) fp32 on the device, ``images`` optional, everything else passed
    through) that returns a new dict with new tensors.  Five launches whatever B and C are (csrc/sp_augment.hip): the noise
    of all 3 * B * channels fields, three filter passes over all of them, one warp of every channel volume (which also
    reads a flipped sample mirrored).  Channels that are flipped but not deformed (images without ``apply_to_images``) take
    one ``torch.where`` over the batch.  There is no CPU path.

    ``flip``: ``None``; ``"random"`` -- one ``random.random() > 0.5`` toss per sample in sample order, as ``HemisphericFlip``
    draws them; or a number ``split_id`` -- samples whose ``case_id`` is above it, as ``HemisphericFlipFixedToCaseId``.

    ``noise="philox"``: ``sp_rng_uniform_pm1`` with (``seed``, call) -- ``seed`` defaults to a clock seed like the reference's,
    the call counter starts at 0 and advances by one per batch, field ``((b * Ctot) + c) * 3 + d`` (deformed label channels
    first, then deformed image channels; d = dx, dy, dz): an augmented run is reproducible from ``seed`` alone.
    ``noise="host"``: one ``numpy.random.RandomState`` per sample, drawn from in the per-sample path's order ((n0, n1, n2)
    arrays, stored transposed), uploaded in one copy: the batch then equals ``HemisphericFlip -> ElasticDeform -> ToTensor ->
    stack`` on the same generator states.  ``__call__(batch, random_states=, flips=)`` fixes the states / flags (tests)."""

    def __init__(self, alpha=100, sigma=4, apply_to_images=False, flip=None, noise="philox", seed=None):
        if not (flip is None or flip == "random" or (isinstance(flip, (int, float)) and not isinstance(flip, bool))):
            raise ValueError("BatchElasticDeform: flip is None, 'random' or a split case id, got %r" % (flip,))
        if noise not in ("philox", "host"):
            raise ValueError("BatchElasticDeform: noise is 'philox' or 'host', got %r" % (noise,))
        self._alpha, self._sigma, self._apply_to_images, self._flip, self._noise = alpha, sigma, apply_to_images, flip, noise
        if seed is None:
            seed = datetime.datetime.now().second + datetime.datetime.now().microsecond
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._calls = 0

    def _flags(self, batch, B):
        if self._flip is None:
            return None
        if self._flip == "random":
            return [random.random() > 0.5 for _ in range(B)]
        return [int(c) > self._flip for c in batch[KEY_CASE_ID]]

    def _host_noise(self, B, n_ch, shape_zyx, random_states):
        Z, Y, X = shape_zyx
        noise = np.empty((B, n_ch, 3, Z, Y, X), dtype=np.float32)
        for b in range(B):
            rs = random_states[b] if random_states is not None else None
            if rs is None:
                rs = np.random.RandomState(datetime.datetime.now().second + datetime.datetime.now().microsecond)
            for c in range(n_ch):
                for d in range(3):
                    noise[b, c, d] = (rs.rand(X, Y, Z) * 2 - 1).astype(np.float32).transpose(2, 1, 0)
        return torch.from_numpy(noise)

    def __call__(self, batch, random_states=None, flips=None):
        from stroke_prediction_amd.runtime import lib as L, ops as O
        labels = batch[KEY_LABELS]
        _require_cuda(labels, "BatchElasticDeform")
        if labels.dim() != 5:
            raise ValueError("BatchElasticDeform needs (B, C, Z, Y, X) labels, got %r" % (tuple(labels.shape),))
        B, C, Z, Y, X = labels.shape
        if X != Y:
            raise ValueError("elastic_transform needs (n, n, d) volumes (data.py:336-337), got (x, y, z) = %r" % ((X, Y, Z),))
        images = batch.get(KEY_IMAGES, [])
        has_images = _present(images)
        if has_images:
            _require_cuda(images, "BatchElasticDeform")
        warp_images = bool(self._apply_to_images and has_images)
        if warp_images and tuple(images.shape[0:1] + images.shape[2:]) != (B, Z, Y, X):
            raise ValueError("BatchElasticDeform: images %r do not match labels %r" % (tuple(images.shape), tuple(labels.shape)))
        if flips is None:
            flips = self._flags(batch, B)
        if flips is not None and len(flips) != B:
            raise ValueError("BatchElasticDeform: %d flip flags for a batch of %d" % (len(flips), B))
        dev = labels.device
        flip_dev = torch.tensor([int(bool(f)) for f in flips], dtype=torch.int32).to(dev) if flips is not None and any(flips) else None
        src0 = labels.contiguous().float()
        src1 = images.contiguous().float() if warp_images else None
        C1 = src1.shape[1] if warp_images else 0
        n_ch, per_field = C + C1, Z * Y * X
        if self._noise == "philox":
            noise = torch.empty((B, n_ch, 3, Z, Y, X), dtype=torch.float32, device=dev)
            call = self._calls & 0xFFFFFFFFFFFFFFFF
            self._calls += 1
            as_i64 = lambda u: u - (1 << 64) if u >= (1 << 63) else u
            L.call("sp_rng_uniform_pm1", O.ptr(noise), B * n_ch * 3, per_field, as_i64(self._seed), as_i64(call), O.stream())
        else:
            noise = self._host_noise(B, n_ch, (Z, Y, X), random_states).to(dev)
        fields, tmp = torch.empty_like(noise), torch.empty_like(noise)
        L.call("sp_gaussian_filter3d_batch", O.ptr(noise), O.ptr(fields), O.ptr(tmp), B * n_ch * 3, Z, Y, X, float(self._sigma), 4.0,
               O.stream())
        dst0 = torch.empty_like(src0)
        dst1 = torch.empty_like(src1) if warp_images else None
        L.call("sp_elastic_warp_batch", O.ptr(src0), O.ptr(dst0), C, O.ptr(src1) if warp_images else None,
               O.ptr(dst1) if warp_images else None, C1, O.ptr(fields), O.ptr(flip_dev) if flip_dev is not None else None, B, Z, Y, X,
               float(self._alpha), float(self._alpha) * 0.22, O.stream())
        out = dict(batch)
        out[KEY_LABELS] = dst0
        if warp_images:
            out[KEY_IMAGES] = dst1
        elif has_images and flip_dev is not None:
            out[KEY_IMAGES] = torch.where(flip_dev.bool().view(B, 1, 1, 1, 1), torch.flip(images, (-1,)), images)
        return out


class ResamplePlaneXY(object):
    """Down- or upsample every (x, y) slice (data.py:354-381): nearest neighbour (``ndi.zoom(order=0)``) or, with
    ``mode='bilinear'``, first order.  ``scipy.ndimage.zoom`` maps output index ``o`` to input coordinate
    ``o * (n_in - 1) / (n_out - 1)`` with ``n_out = round(n_in * factor)``; order 0 takes ``floor(c + 0.5)``, order 1
    interpolates between the two neighbours.  Index arithmetic on whatever the sample holds (device tensors or numpy)."""

    def __init__(self, scale_factor=1, mode='nearest'):
        self._scale_factor = scale_factor
        self._order = 1 if mode == 'bilinear' else 0

    def _axis(self, n_in, device):
        n_out = int(round(n_in * self._scale_factor))
        if n_out == n_in:
            return None
        c = torch.arange(n_out, dtype=torch.float64, device=device) * ((n_in - 1) / max(n_out - 1, 1))
        return c

    def _resample(self, vol):
        if self._scale_factor == 1:
            return vol
        was_numpy = isinstance(vol, np.ndarray)
        t = torch.from_numpy(np.ascontiguousarray(vol)) if was_numpy else vol
        for axis in (0, 1):
            c = self._axis(t.shape[axis], t.device)
            if c is None:
                continue
            if self._order == 0:
                t = t.index_select(axis, torch.floor(c + 0.5).long().clamp_(0, t.shape[axis] - 1))
            else:
                lo = torch.floor(c).long().clamp_(0, t.shape[axis] - 1)
                hi = (lo + 1).clamp_(max=t.shape[axis] - 1)
                w = (c - lo.double()).to(t.dtype if t.is_floating_point() else torch.float32)
                shape = [1] * t.dim()
                shape[axis] = -1
                a, b = t.index_select(axis, lo).float(), t.index_select(axis, hi).float()
                t = (a + (b - a) * w.view(shape)).to(t.dtype if t.is_floating_point() else torch.float32)
        return t.numpy() if was_numpy else t

    def __call__(self, sample):
        result = emptyCopyFromSample(sample)
        result[KEY_GLOBAL] = sample[KEY_GLOBAL]
        for k in (KEY_IMAGES, KEY_LABELS):
            if _present(sample[k]):
                result[k] = self._resample(sample[k])
        return result


class Compose(object):
    """``torchvision.transforms.Compose`` for sample dicts (the reference's loader factories wrap their transform lists
    in it, data.py:121-124).  ``device``: numpy samples are uploaded once before the first transform (``to_device``), so
    the whole chain runs on device tensors; ``None`` leaves them where they are (host pipelines, CPU tests)."""

    def __init__(self, transforms, device=None):
        self.transforms = list(transforms)
        self.device = device

    def __call__(self, sample):
        if self.device is not None:
            sample = to_device(sample, self.device)
        for t in self.transforms:
            sample = t(sample)
        return sample


# ---------------------------------------------------------------------------------------------- datasets and loaders
# The reference reads a private 29-subject NIfTI + CSV data set from hard-wired paths (data.py:30-99).  The loader
# factories below keep its signatures (data.py:113-212) and the batch-dict contract; the samples come from
# ``StrokeLindaDataset3D`` when that data set is reachable (nibabel importable and the root directory present), and from
# ``SyntheticStrokeDataset3D`` -- deterministic blob volumes of the same shapes and channel meanings -- otherwise.

N_SYNTHETIC_CASES = 29


def _blob_field(rng, shape, sigma):
    """smoothed uniform noise in [0, 1], low resolution (cheap on the host)"""
    from scipy.ndimage import gaussian_filter
    f = gaussian_filter(rng.rand(*shape), sigma, mode="constant")
    f -= f.min()
    return f / max(float(f.max()), 1e-12)


def synthetic_sample(case_id, xy=256, z=28, n_modalities=2, n_labels=3, n_globals=5):
    """One case in the reference's sample layout: ``images`` (x, y, z, n_modalities), ``labels`` (x, y, z, n_labels) --
    nested binary blobs core < follow-up lesion < penumbra -- and ``clinical`` (1, 1, 1, n_globals) =
    (tO->tA, tA->tR, NIHSS, sex, age).  Deterministic in ``case_id``."""
    rng = np.random.RandomState(7919 + int(case_id))
    low = max(8, xy // 4)
    up = xy // low
    f = _blob_field(rng, (low, low, z), (3.0, 3.0, 2.0))
    thr = np.quantile(f, [0.93, 0.80, 0.86])                 # core, penumbra, lesion: core < lesion < penumbra as sets
    big = lambda a: np.repeat(np.repeat(a, up, axis=0), up, axis=1)
    labels = np.stack([big(f > thr[0]), big(f > thr[1]), big(f > thr[2])], axis=3)[..., :n_labels].astype(np.float32)
    imgs = [big(_blob_field(rng, (low, low, z), (2.0, 2.0, 1.0))) * s for s in (12.0, 40.0)][:n_modalities]
    images = np.stack(imgs, axis=3).astype(np.float32) if imgs else []
    clinical = np.array([rng.uniform(0.5, 4.0), rng.uniform(0.5, 5.0), float(rng.randint(0, 25)), float(rng.randint(0, 2)),
                         rng.uniform(40, 90)][:n_globals]).reshape((1, 1, 1, n_globals))
    return {KEY_CASE_ID: int(case_id), KEY_IMAGES: images, KEY_LABELS: labels, KEY_GLOBAL: clinical}


def synthetic_shape_batch(batch, d=28, hw=128, seed=0):
    """A ready batch for the CAE path (bench.py, smoke tests): ``labels`` (B, 3, d, hw, hw) binary blobs and
    ``clinical`` (B, 5, 1, 1, 1), i.e. ``ToTensor()``-layout samples of ``synthetic_sample`` stacked."""
    labels, clinical = [], []
    for b in range(batch):
        s = synthetic_sample(seed * 131 + b, xy=hw, z=d, n_modalities=0)
        labels.append(torch.from_numpy(s[KEY_LABELS]).permute(3, 2, 1, 0))
        clinical.append(torch.from_numpy(s[KEY_GLOBAL].astype(np.float32)).permute(3, 2, 1, 0))
    return torch.stack(labels).contiguous(), torch.stack(clinical).contiguous()


class SyntheticStrokeDataset3D(torch.utils.data.Dataset):
    """Stand-in for ``StrokeLindaDataset3D`` (data.py:30-99): same ``__getitem__`` contract, synthetic content."""

    def __init__(self, modalities=[], labels=[], transform=None, single_case_id=None, xy=256, z=28, n_cases=N_SYNTHETIC_CASES):
        self._modalities, self._labels, self._transform = modalities, labels, transform
        self._xy, self._z = xy, z
        self._item_index_map = [{KEY_CASE_ID: c, KEY_CLINICAL_IDX: c - 1} for c in range(1, n_cases + 1)
                                if single_case_id is None or single_case_id == c]

    def __len__(self):
        return len(self._item_index_map)

    def __getitem__(self, item):
        case_id = self._item_index_map[item][KEY_CASE_ID]
        result = synthetic_sample(case_id, self._xy, self._z, n_modalities=min(2, len(self._modalities)),
                                  n_labels=min(3, len(self._labels)) if self._labels else 0)
        if not self._labels:
            result[KEY_LABELS] = []
        if self._transform:
            result = self._transform(result)
        return result


class StrokeLindaDataset3D(torch.utils.data.Dataset):
    """The reference's NIfTI + CSV data set (data.py:30-99): ``<root>/<case>/train<case><suffix>.nii.gz`` volumes and one
    CSV row of clinical values per case.  Needs nibabel and the (private) data; see ``dataset_available``."""
    PATH_ROOT = '/share/data_zoe1/lucas/Linda_Segmentations'
    PATH_CSV = '/share/data_zoe1/lucas/Linda_Segmentations/clinical_cleaned.csv'

    def __init__(self, root_dir=PATH_ROOT, modalities=[], labels=[], clinical=PATH_CSV, transform=None, single_case_id=None):
        import csv
        self._root_dir, self._modalities, self._labels, self._transform = root_dir, modalities, labels, transform
        with open(clinical, 'r') as f:
            self._clinical = list(csv.reader(f, delimiter=','))[1:]            # one header row
        self._item_index_map = [{KEY_CASE_ID: int(row[0]), KEY_CLINICAL_IDX: i} for i, row in enumerate(self._clinical)
                                if single_case_id is None or single_case_id == int(row[0])]

    def _volume(self, case_id, suffix):
        import os
        import nibabel as nib
        fn = os.path.join(self._root_dir, '{1}/{0}{1}{2}.nii.gz'.format('train', str(case_id), suffix))
        return np.asarray(nib.load(fn).get_fdata())[:, :, :, np.newaxis]

    def __len__(self):
        return len(self._item_index_map)

    def __getitem__(self, item):
        entry = self._item_index_map[item]
        case_id = entry[KEY_CASE_ID]
        values = [float(v) for v in self._clinical[entry[KEY_CLINICAL_IDX]][1:]]
        result = {KEY_CASE_ID: case_id, KEY_IMAGES: [], KEY_LABELS: [], KEY_GLOBAL: []}
        if values:
            result[KEY_GLOBAL] = np.array(values).reshape((1, 1, 1, len(values)))
        for key, names in ((KEY_LABELS, self._labels), (KEY_IMAGES, self._modalities)):
            if names:
                result[key] = np.concatenate([self._volume(case_id, n) for n in names], axis=DIM_CHANNEL_NUMPY_3D)
        return self._transform(result) if self._transform else result


def dataset_available():
    import os
    if os.environ.get("SP_SYNTHETIC_DATA"):
        return False
    try:
        import nibabel  # noqa: F401
    except Exception:
        return False
    return os.path.isdir(StrokeLindaDataset3D.PATH_ROOT) and os.path.isfile(StrokeLindaDataset3D.PATH_CSV)


def _dataset(modalities, labels, transform_list, device):
    tf = Compose(transform_list, device=device)
    if dataset_available():
        return StrokeLindaDataset3D(modalities=modalities, labels=labels, transform=tf)
    return SyntheticStrokeDataset3D(modalities=modalities, labels=labels, transform=tf)


def _pipeline_device():
    """the transform chain runs on the GPU when there is one (ElasticDeform / PadImages are HIP / device ops)"""
    return "cuda" if torch.cuda.is_available() else None


def set_np_seed(workerid):
    np.random.seed(torch.initial_seed() % np.iinfo(np.int32).max)


class _CollateThenTransform(object):
    """``collate_fn`` of a loader with a ``batch_transform``: the default collate, then the transform on the collated batch"""

    def __init__(self, batch_transform):
        self.batch_transform = batch_transform

    def __call__(self, samples):
        from torch.utils.data import default_collate
        return self.batch_transform(default_collate(samples))


def _loader(dataset, items, batch_size, num_workers, pin_memory, seeded, batch_transform=None):
    from torch.utils.data import DataLoader
    from torch.utils.data.sampler import SubsetRandomSampler
    if getattr(getattr(dataset, "transform", None), "device", None) is not None:
        num_workers = 0      # the transform chain uploads and runs HIP kernels: a forked worker cannot re-initialise the GPU
    extra = dict(collate_fn=_CollateThenTransform(batch_transform)) if batch_transform is not None else {}
    return DataLoader(dataset, batch_size=batch_size, sampler=SubsetRandomSampler(items), num_workers=num_workers,
                      pin_memory=pin_memory, worker_init_fn=set_np_seed if seeded else None, **extra)


def _fold_items(dataset, indices, shuffle, random_seed):
    items = sorted(set(range(len(dataset))) & set(indices))
    if shuffle:
        np.random.RandomState(random_seed).shuffle(items)
    return items


# ---------------------------------------------------------------------------------------------- device-resident case cache
# The loaders above prepare every sample of every batch from scratch: decode (or synthesise) the case, upload it, resample, flip,
# pad, cut, stack.  ``device_cache=True`` on the factories uploads every case ONCE (``DeviceCaseCache``) and builds a batch with one
# launch of ``sp_patch_gather_batch`` (csrc/sp_gather.hip) from a small table of (case, origin, flip) rows (``CachedBatchLoader``).

class DeviceCaseCache(object):
    """Every case of ``dataset`` (or its ``items``) on ``device``, read once.  ``dataset`` carries the deterministic prefix of the
    transform chain only (``ResamplePlaneXY``, uploading through ``Compose(device=...)`` as the loaders do), so the cached values are
    those ``to_device`` -> ``ResamplePlaneXY`` -> ``ToTensor`` give: ``images`` (N, C0, Z, Y, X) and ``labels`` (N, C1, Z, Y, X) fp32
    with X contiguous, ``clinical`` (N, G, 1, 1, 1); an absent group is ``None``.  ``case_ids`` / ``clinical_idx``: per slot;
    ``slot_of[item]``: the slot of a data set item.  All cases must have the same extents."""

    def __init__(self, dataset, device="cuda", items=None):
        self.dataset, self.device = dataset, device
        self.items = list(range(len(dataset))) if items is None else sorted(set(int(i) for i in items))
        if not self.items:
            raise ValueError("DeviceCaseCache: no cases to cache")
        self.slot_of = {item: n for n, item in enumerate(self.items)}
        self.case_ids, self.clinical_idx = [], []
        self.images = self.labels = self.clinical = None
        stores = {KEY_IMAGES: None, KEY_LABELS: None, KEY_GLOBAL: None}
        for n, item in enumerate(self.items):
            sample = to_device(dataset[item], device) if device is not None else dataset[item]
            self.case_ids.append(int(sample[KEY_CASE_ID]))
            self.clinical_idx.append(sample.get(KEY_CLINICAL_IDX, 0))
            for k in stores:
                v = sample.get(k, [])
                if not _present(v):
                    if stores[k] is not None:
                        raise ValueError("DeviceCaseCache: case %d has no %s, earlier cases have" % (self.case_ids[-1], k))
                    continue
                v = (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).float().permute(3, 2, 1, 0)
                if stores[k] is None:
                    if n:
                        raise ValueError("DeviceCaseCache: case %d has %s, earlier cases have none" % (self.case_ids[-1], k))
                    stores[k] = torch.empty((len(self.items),) + tuple(v.shape), dtype=torch.float32, device=v.device)
                if tuple(v.shape) != tuple(stores[k].shape[1:]):
                    raise ValueError("DeviceCaseCache: %s of case %d are (c, z, y, x) = %r, those of case %d %r: all cases must have the "
                                     "same extents" % (k, self.case_ids[-1], tuple(v.shape), self.case_ids[0], tuple(stores[k].shape[1:])))
                stores[k][n].copy_(v)
        self.images, self.labels, self.clinical = stores[KEY_IMAGES], stores[KEY_LABELS], stores[KEY_GLOBAL]
        if self.images is None and self.labels is None:
            raise ValueError("DeviceCaseCache: the data set yields neither images nor labels")
        if self.images is not None and self.labels is not None and self.images.shape[2:] != self.labels.shape[2:]:
            raise ValueError("DeviceCaseCache: images %r and labels %r differ in extents" % (tuple(self.images.shape), tuple(self.labels.shape)))
        self.shape_zyx = tuple((self.images if self.images is not None else self.labels).shape[2:])
        self._fg_index = {}

    def __len__(self):
        return len(self.items)

    def foreground_index(self, channels=None, threshold=0.5):
        """The row index of the cases' foreground voxels (``sp_fg_row_index``, csrc/sp_fgpatch.hip): int32 (N, Z * Y + 1) on the
        device, the exclusive prefix sum of the per-x-row counts of the voxels whose label exceeds ``threshold`` in one of
        ``channels`` (``None``: any label channel); the last column is the case's total.  Built on first use -- two launches, no host
        read -- and kept per (channel mask, threshold); writing to ``labels`` afterwards makes it stale."""
        if self.labels is None:
            raise ValueError("DeviceCaseCache.foreground_index: the cache holds no labels")
        from stroke_prediction_amd.runtime import lib as L, ops as O
        C1 = int(self.labels.shape[1])
        key = (_chanmask(channels, C1, "DeviceCaseCache.foreground_index"), float(threshold))
        prefix = self._fg_index.get(key)
        if prefix is None:
            _require_cuda(self.labels, "DeviceCaseCache.foreground_index")
            Z, Y, X = self.shape_zyx
            prefix = torch.empty((len(self), Z * Y + 1), dtype=torch.int32, device=self.labels.device)
            L.call("sp_fg_row_index", O.ptr(self.labels), len(self), C1, Z, Y, X, _as_i32(key[0]), key[1], O.ptr(prefix), O.stream())
            self._fg_index[key] = prefix
        return prefix

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.images, self.labels, self.clinical) if t is not None)


def _chanmask(channels, C1, who):
    """label channels -> the bit mask of the foreground kernels (``None``: all ``C1`` channels)"""
    if C1 > 32:
        raise ValueError("%s: %d label channels, the channel mask has 32 bits" % (who, C1))
    if channels is None:
        return (1 << C1) - 1
    mask = 0
    for c in channels:
        if not 0 <= int(c) < C1:
            raise ValueError("%s: channel %d of %d label channels" % (who, int(c), C1))
        mask |= 1 << int(c)
    if not mask:
        raise ValueError("%s: no channel selected" % who)
    return mask


def _as_i32(u):
    """the 32 bits of an unsigned word as the int32 the C ABI takes"""
    return u - (1 << 32) if u >= (1 << 31) else u


class ForegroundOversample(object):
    """Foreground oversampling of the patches a ``CachedBatchLoader`` cuts: with probability ``fraction`` (nnU-Net uses a third) a
    sample's uniformly drawn patch origin is replaced by one that puts a uniformly drawn FOREGROUND voxel of its case at a uniformly
    drawn position ``j`` of the label patch.  A voxel is foreground when its label exceeds ``threshold`` in one of ``channels``
    (``None``: any label channel).  The voxel is picked on the device (``sp_patch_origins_fg``, csrc/sp_fgpatch.hip) from the cached
    labels through ``DeviceCaseCache.foreground_index``: one small launch per batch in front of the gather, no host read.  The
    origin is ``o = clamp(f - j, 0, padded - patch)`` with ``f`` the voxel in the (flipped) label frame, so the voxel sits at ``j``
    unless a clamp acts and inside the label patch either way; a case without foreground keeps its uniform origin.  Under a
    ``PatchAugment`` the voxel sits at ``j`` BEFORE the transform: rotation, scaling and deformation may move it out of the patch,
    and the guarantee is statistical, not per sample.

    Every draw comes from this object's own ``numpy.random.RandomState(seed)`` -- the same number of draws per batch whatever the
    tosses say -- never from Python's ``random``: the loader's origin and flip draws stay where they are."""

    def __init__(self, fraction=1.0 / 3.0, channels=None, threshold=0.5, seed=None):
        if not 0 <= fraction <= 1:
            raise ValueError("ForegroundOversample: fraction is a probability, got %r" % (fraction,))
        if channels is not None:
            channels = [int(c) for c in channels]
            if any(c < 0 for c in channels) or len(set(channels)) != len(channels):
                raise ValueError("ForegroundOversample: channels are distinct non-negative label channel indices, got %r" % (channels,))
            if not channels:
                raise ValueError("ForegroundOversample: channels is None (all label channels) or a non-empty list")
        self.fraction, self.channels, self.threshold = float(fraction), channels, float(threshold)
        if seed is None:
            seed = datetime.datetime.now().second + datetime.datetime.now().microsecond
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._rs = np.random.RandomState(self._seed & 0xFFFFFFFF)

    def draw(self, B, ext1):
        """The host draws of one batch, int32 (B, 5): ``force`` (toss < fraction), ``u`` (a uniform 32-bit word, stored as the int32
        of the same bits), ``jx, jy, jz`` uniform in [0, ext1) per axis."""
        r = self._rs.random_sample((B, 5))                 # toss, word, three positions: 53-bit fractions k / 2^53
        ext = np.asarray(ext1, dtype=np.int32)
        draws = np.empty((B, 5), dtype=np.int32)
        draws[:, 0] = r[:, 0] < self.fraction
        draws[:, 1] = (r[:, 1] * 4294967296.0).astype(np.uint32).view(np.int32)      # floor(k / 2^21): every word equally likely
        draws[:, 2:5] = np.minimum((r[:, 2:5] * ext).astype(np.int32), ext - 1)
        return draws


def _origins_fg_launch(cache, foreground, table_dev, draws_dev, ext1, omax):
    """``sp_patch_origins_fg`` on the stream of the upload and the gather: rewrites the origins of ``table_dev`` in place"""
    import ctypes
    from stroke_prediction_amd.runtime import lib as L, ops as O
    Z, Y, X = cache.shape_zyx
    C1 = int(cache.labels.shape[1])
    mask = _chanmask(foreground.channels, C1, "CachedBatchLoader")
    prefix = cache.foreground_index(foreground.channels, foreground.threshold)
    i3 = lambda v: (ctypes.c_int32 * 3)(*[int(a) for a in v])
    L.call("sp_patch_origins_fg", O.ptr(cache.labels), O.ptr(prefix), len(cache), C1, Z, Y, X, _as_i32(mask), foreground.threshold,
           O.ptr(draws_dev), i3(ext1), i3(omax), O.ptr(table_dev), None, int(table_dev.shape[0]), O.stream())


def _gather_launch(cache, table, ext0, pad0, padval0, ext1, pad1, foreground=None, omax=None):
    """The one ``sp_patch_gather_batch`` launch of a batch: ``table`` (host int32 (B, 5): slot, ox, oy, oz, flip) goes up in one small
    pinned copy; returns (images (B, C0, d0, h0, w0) or ``[]``, labels (B, C1, d1, h1, w1) or ``[]``, the device table).  With
    ``foreground`` (a ``ForegroundOversample``; ``omax`` = padded - ext0) the same copy also carries its draws and ``sp_patch_origins_fg``
    rewrites the device table between the copy and the gather."""
    import ctypes
    from stroke_prediction_amd.runtime import lib as L, ops as O
    src0, src1 = cache.images, cache.labels
    _require_cuda(src0 if src0 is not None else src1, "CachedBatchLoader")
    dev = (src0 if src0 is not None else src1).device
    B = int(table.shape[0])
    Z, Y, X = cache.shape_zyx
    if foreground is None:
        table_dev = table.pin_memory().to(dev, non_blocking=True)
    else:
        host = torch.from_numpy(np.concatenate((table.numpy().reshape(-1), foreground.draw(B, ext1).reshape(-1))))
        words = host.pin_memory().to(dev, non_blocking=True)
        table_dev = words[:B * 5].view(B, 5)
        _origins_fg_launch(cache, foreground, table_dev, words[B * 5:], ext1, omax)
    dst0 = torch.empty((B, src0.shape[1], ext0[2], ext0[1], ext0[0]), dtype=torch.float32, device=dev) if src0 is not None else None
    dst1 = torch.empty((B, src1.shape[1], ext1[2], ext1[1], ext1[0]), dtype=torch.float32, device=dev) if src1 is not None else None
    i3 = lambda v: (ctypes.c_int32 * 3)(*[int(a) for a in v])
    L.call("sp_patch_gather_batch", O.ptr(src0), O.ptr(dst0), src0.shape[1] if src0 is not None else 0, i3(ext0), i3(pad0), float(padval0),
           O.ptr(src1), O.ptr(dst1), src1.shape[1] if src1 is not None else 0, i3(ext1), i3(pad1), 0.0, O.ptr(table_dev), len(cache), B,
           Z, Y, X, O.stream())
    return (dst0 if dst0 is not None else []), (dst1 if dst1 is not None else []), table_dev


class PatchAugment(object):
    """Per-sample augmentation of the patches a ``CachedBatchLoader`` cuts, applied INSIDE the launch that builds the batch
    (``sp_patch_sample_batch``, csrc/sp_sample.hip): the cache is read through an output -> source map instead of at an origin, so a
    rotation pulls in the voxels outside the patch and images (the padded patch) and labels (its valid-convolution crop) move through
    the same map although their extents differ.

    Per sample: with ``p_affine`` a rotation about the z axis by an angle in +-``rotate_deg`` and one in-plane scale ``s`` in
    ``scale`` -- ``M = (1 / s) R(angle)`` on the (x, y) block and 1 on z (thick slices: no out-of-plane rotation, z is not scaled);
    with ``p_elastic`` the displacement of ``ElasticDeform`` / ``BatchElasticDeform`` (uniform noise in [-1, 1), Gaussian filter
    ``sigma``, scaled by ``alpha`` in plane and ``0.22 alpha`` along z) on the image patch's grid, one field triple shared by all
    channels of both groups; with ``p_intensity`` a gain in ``gain`` and a bias in ``bias`` per image channel (padding keeps its
    value).  ``label_threshold``: labels are 1.0 where the interpolated value reaches it, else 0.0 (``None``: left interpolated).

    Every host draw comes from this object's own ``numpy.random.RandomState(seed)`` -- the same number of draws per batch whatever
    the tosses say -- never from Python's ``random``: the loader's origin and flip draws stay where they are.  The noise comes from
    ``sp_rng_uniform_pm1`` with (``seed``, call), the call counter advancing by one per batch as in ``BatchElasticDeform``; it and the
    three filter passes are skipped for a batch in which no sample deforms.  A run is reproducible from ``seed`` alone."""

    def __init__(self, rotate_deg=15.0, scale=(0.85, 1.15), alpha=100, sigma=4, gain=(0.9, 1.1), bias=(-0.1, 0.1),
                 p_affine=0.5, p_elastic=0.5, p_intensity=0.5, label_threshold=0.5, seed=None):
        for name, pair in (("scale", scale), ("gain", gain), ("bias", bias)):
            if len(pair) != 2 or not pair[0] <= pair[1]:
                raise ValueError("PatchAugment: %s is a (low, high) pair, got %r" % (name, pair))
        if not scale[0] > 0:
            raise ValueError("PatchAugment: scale must be positive, got %r" % (scale,))
        for name, p in (("p_affine", p_affine), ("p_elastic", p_elastic), ("p_intensity", p_intensity)):
            if not 0 <= p <= 1:
                raise ValueError("PatchAugment: %s is a probability, got %r" % (name, p))
        self.rotate_deg, self.scale, self.alpha, self.sigma, self.gain, self.bias = float(rotate_deg), tuple(scale), alpha, sigma, tuple(gain), tuple(bias)
        self.p_affine, self.p_elastic, self.p_intensity = p_affine, p_elastic, p_intensity
        self.label_threshold = label_threshold
        if seed is None:
            seed = datetime.datetime.now().second + datetime.datetime.now().microsecond
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._rs = np.random.RandomState(self._seed & 0xFFFFFFFF)
        self._calls = 0

    @property
    def thresh1(self):
        """the ``thresh1`` argument of ``sp_patch_sample_batch``"""
        return -1.0 if self.label_threshold is None else float(self.label_threshold)

    def draw(self, B, C0):
        """The host draws of one batch: ``xform`` (B, 16) fp32 (M[9], t[3], alpha_xy, alpha_z, two reserved words), ``intensity``
        (B, C0, 2) fp32 (gain, bias) or ``None`` when no sample changes intensity (or there are no image channels), ``elastic``
        (B,) bool, ``call``: the noise call counter of this batch."""
        rs = self._rs
        toss = rs.rand(B, 3)
        angle = np.deg2rad(rs.uniform(-self.rotate_deg, self.rotate_deg, B))
        s = rs.uniform(self.scale[0], self.scale[1], B)
        gain = rs.uniform(self.gain[0], self.gain[1], (B, max(C0, 1)))
        bias = rs.uniform(self.bias[0], self.bias[1], (B, max(C0, 1)))
        affine, elastic, inten = toss[:, 0] < self.p_affine, toss[:, 1] < self.p_elastic, toss[:, 2] < self.p_intensity
        xform = np.zeros((B, 16), dtype=np.float32)
        xform[:, 0] = xform[:, 4] = xform[:, 8] = 1.0
        for b in np.nonzero(affine)[0]:
            c, sn = np.cos(angle[b]) / s[b], np.sin(angle[b]) / s[b]
            xform[b, 0:2] = (c, -sn)
            xform[b, 3:5] = (sn, c)
        xform[elastic, 12] = float(self.alpha)
        xform[elastic, 13] = float(self.alpha) * 0.22
        intensity = None
        if C0 > 0 and inten.any():
            intensity = np.empty((B, C0, 2), dtype=np.float32)
            intensity[:, :, 0] = np.where(inten[:, None], gain[:, :C0], 1.0)
            intensity[:, :, 1] = np.where(inten[:, None], bias[:, :C0], 0.0)
        call = self._calls
        self._calls += 1
        return {"xform": xform, "intensity": intensity, "elastic": elastic, "call": call}

    def make_fields(self, draws, B, grid_zyx, device):
        """(B, 3, d0, h0, w0) filtered noise on the image patch's grid (two launch groups: rng, three filter passes), or ``None``
        when no sample of the batch deforms."""
        if not draws["elastic"].any():
            return None
        from stroke_prediction_amd.runtime import lib as L, ops as O
        d0, h0, w0 = grid_zyx
        noise = torch.empty((B, 3, d0, h0, w0), dtype=torch.float32, device=device)
        as_i64 = lambda u: u - (1 << 64) if u >= (1 << 63) else u
        L.call("sp_rng_uniform_pm1", O.ptr(noise), B * 3, d0 * h0 * w0, as_i64(self._seed), as_i64(draws["call"] & 0xFFFFFFFFFFFFFFFF),
               O.stream())
        fields, tmp = torch.empty_like(noise), torch.empty_like(noise)
        L.call("sp_gaussian_filter3d_batch", O.ptr(noise), O.ptr(fields), O.ptr(tmp), B * 3, d0, h0, w0, float(self.sigma), 4.0, O.stream())
        return fields


def _sample_launch(cache, table, ext0, pad0, padval0, ext1, pad1, augment, foreground=None, omax=None):
    """``_gather_launch`` through ``augment``: one pinned upload carries the table, ``xform`` and ``intensity`` (int32 and fp32 words
    of one buffer), ``sp_patch_sample_batch`` builds the batch; the noise and filter launches come first when a sample deforms.
    ``foreground`` / ``omax``: as for ``_gather_launch``; its draws are the last words of the upload."""
    import ctypes
    from stroke_prediction_amd.runtime import lib as L, ops as O
    src0, src1 = cache.images, cache.labels
    _require_cuda(src0 if src0 is not None else src1, "CachedBatchLoader")
    dev = (src0 if src0 is not None else src1).device
    B = int(table.shape[0])
    Z, Y, X = cache.shape_zyx
    C0 = src0.shape[1] if src0 is not None else 0
    draws = augment.draw(B, C0)
    inten = draws["intensity"]
    n_aug = B * 21 + (B * C0 * 2 if inten is not None else 0)
    host = torch.empty(n_aug + (B * 5 if foreground is not None else 0), dtype=torch.int32)
    host[:B * 5] = table.reshape(-1)
    host[B * 5:B * 21].view(torch.float32).copy_(torch.from_numpy(draws["xform"]).reshape(-1))
    if inten is not None:
        host[B * 21:n_aug].view(torch.float32).copy_(torch.from_numpy(inten).reshape(-1))
    if foreground is not None:
        host[n_aug:].copy_(torch.from_numpy(foreground.draw(B, ext1)).reshape(-1))
    words = host.pin_memory().to(dev, non_blocking=True)
    table_dev = words[:B * 5].view(B, 5)
    xform_dev = words[B * 5:B * 21].view(torch.float32)
    inten_dev = words[B * 21:n_aug].view(torch.float32) if inten is not None else None
    if foreground is not None:
        _origins_fg_launch(cache, foreground, table_dev, words[n_aug:], ext1, omax)
    fields = augment.make_fields(draws, B, (ext0[2], ext0[1], ext0[0]), dev)
    dst0 = torch.empty((B, C0, ext0[2], ext0[1], ext0[0]), dtype=torch.float32, device=dev) if src0 is not None else None
    dst1 = torch.empty((B, src1.shape[1], ext1[2], ext1[1], ext1[0]), dtype=torch.float32, device=dev) if src1 is not None else None
    i3 = lambda v: (ctypes.c_int32 * 3)(*[int(a) for a in v])
    L.call("sp_patch_sample_batch", O.ptr(src0), O.ptr(dst0), C0, i3(ext0), i3(pad0), float(padval0),
           O.ptr(src1), O.ptr(dst1), src1.shape[1] if src1 is not None else 0, i3(ext1), i3(pad1), augment.thresh1, O.ptr(table_dev),
           O.ptr(xform_dev), O.ptr(fields) if fields is not None else None, O.ptr(inten_dev) if inten_dev is not None else None,
           len(cache), B, Z, Y, X, O.stream())
    return (dst0 if dst0 is not None else []), (dst1 if dst1 is not None else []), table_dev


def _pair(name, pair, who="IntensityAugment"):
    if len(pair) != 2 or not pair[0] <= pair[1]:
        raise ValueError("%s: %s is a (low, high) pair, got %r" % (who, name, pair))
    return (float(pair[0]), float(pair[1]))


def gaussian_weights(sigma, radius=None, truncate=4.0):
    """The taps of ``scipy.ndimage.gaussian_filter(sigma, truncate)`` (``_gaussian_kernel1d``): ``exp(-x^2 / (2 sigma^2))`` for
    ``x = -r .. r``, ``r = int(truncate sigma + 0.5)``, normalised in float64; centred in a row of ``2 radius + 1`` zeros when a
    larger ``radius`` is given."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi = phi / phi.sum()
    if radius is None or radius == r:
        return phi
    if radius < r:
        raise ValueError("gaussian_weights: sigma %r needs radius %d, got %d" % (sigma, r, radius))
    out = np.zeros(2 * radius + 1)
    out[radius - r:radius + r + 1] = phi
    return out


class IntensityAugment(object):
    """Intensity augmentation of a collated batch on the device, a callable ``batch -> batch`` for ``batch_transform=`` on the loader
    factories: Gaussian blur, Gaussian noise, brightness, contrast and gamma of ``batch['images']`` ((B, C0, Z, Y, X) CUDA fp32), with
    batchgenerators' / nnU-Net's ranges and probabilities as defaults.  Labels and every other key pass through untouched; the
    images come back as a new tensor.  There is no CPU path.  Two launches per batch (``sp_intensity_stats_partials``,
    ``sp_intensity_apply_batch``), five when a field blurs (three passes of ``sp_blur3d_reflect_batch`` first), one pinned upload
    of the parameter table and the blur weights, no host read, no synchronisation (csrc/sp_intensity.hip).

    A field is one (sample, channel) volume.  Tosses are per sample, parameters per field.  The stages, in this fixed order:

    1. blur, ``p_blur`` per sample and then ``p_blur_channel`` per channel: ``scipy.ndimage.gaussian_filter(x, sigma)``
       (``mode="reflect"``, ``truncate=4``), ``sigma`` uniform in ``blur_sigma``.  Every extent must reach the radius ``int(4 sigma + .5)``.
    2. noise, ``p_noise``: ``y + sqrt(variance) n`` with ``variance`` uniform in ``noise_variance`` and ``n`` standard normal (Philox4x32-10
       + Box-Muller keyed by (``seed``, call, field, voxel); the call counter advances by one per batch).
    3. brightness, ``p_gain``: ``g y``, ``g`` uniform in ``gain``.
    4. contrast, ``p_contrast``: ``clamp((y - mean) k + mean, min, max)`` with the field's own mean and range (batchgenerators'
       ``preserve_range=True``); ``k`` below 1 or above 1 with equal probability, uniform in that part of ``contrast``.
    5. gamma: ``((y - min) / (range + 1e-7))^gamma range + min``, ``gamma`` drawn like ``k`` from ``gamma``.  With ``p_gamma_invert``
       the inverted form (the same transform of ``-y``); otherwise with ``p_gamma`` the plain one.  ``retain_stats`` is not implemented.

    Differences from nnU-Net, on purpose: blur comes BEFORE noise (nnU-Net adds the noise first), so that the noise can be
    regenerated from its counter in the statistics pass and in the apply pass instead of being stored; each field takes at most
    one gamma (nnU-Net may apply the inverted and the plain one in a row).  The noise variance is absolute: it assumes inputs
    of roughly unit scale.  Voxels that ``PadImages`` wrote are treated as image -- a batch-level transform cannot tell them
    apart, and batchgenerators treats its padding the same way.

    Every host draw comes from this object's own ``numpy.random.RandomState(seed)`` -- the same number of draws per batch whatever
    the tosses say -- never from Python's ``random``.  A run is reproducible from ``seed`` alone."""

    def __init__(self, noise_variance=(0, 0.1), p_noise=0.1, blur_sigma=(0.5, 1.0), p_blur=0.2, p_blur_channel=0.5,
                 gain=(0.75, 1.25), p_gain=0.15, contrast=(0.75, 1.25), p_contrast=0.15, gamma=(0.7, 1.5), p_gamma=0.3,
                 p_gamma_invert=0.1, seed=None):
        self.noise_variance, self.blur_sigma = _pair("noise_variance", noise_variance), _pair("blur_sigma", blur_sigma)
        self.gain, self.contrast, self.gamma = _pair("gain", gain), _pair("contrast", contrast), _pair("gamma", gamma)
        if self.noise_variance[0] < 0:
            raise ValueError("IntensityAugment: noise_variance must not be negative, got %r" % (noise_variance,))
        for name, pair in (("blur_sigma", self.blur_sigma), ("gain", self.gain), ("contrast", self.contrast), ("gamma", self.gamma)):
            if not pair[0] > 0:
                raise ValueError("IntensityAugment: %s must be positive, got %r" % (name, pair))
        if int(4.0 * self.blur_sigma[1] + 0.5) > 64:
            raise ValueError("IntensityAugment: blur_sigma %r needs a radius above 64" % (blur_sigma,))
        probs = dict(p_noise=p_noise, p_blur=p_blur, p_blur_channel=p_blur_channel, p_gain=p_gain, p_contrast=p_contrast, p_gamma=p_gamma,
                     p_gamma_invert=p_gamma_invert)
        for name, p in probs.items():
            if not 0 <= p <= 1:
                raise ValueError("IntensityAugment: %s is a probability, got %r" % (name, p))
            setattr(self, name, float(p))
        if seed is None:
            seed = datetime.datetime.now().second + datetime.datetime.now().microsecond
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._rs = np.random.RandomState(self._seed & 0xFFFFFFFF)
        self._calls = 0

    def _split_uniform(self, pair, shape):
        """batchgenerators' draw of a contrast factor or a gamma: below 1 or above 1 with equal probability where the range holds
        both, uniform in that part; always the same three draws"""
        rs, (lo, hi) = self._rs, pair
        coin, below, above = rs.rand(*shape), rs.uniform(lo, min(hi, 1.0), shape), rs.uniform(max(lo, 1.0), hi, shape)
        if hi <= 1:
            return below
        if lo >= 1:
            return above
        return np.where(coin < 0.5, below, above)

    def draw(self, B, C0):
        """The host draws of one batch: ``params`` (B * C0, 8) fp32, row ``b * C0 + c`` = [sigma_n, gain, contrast, gamma, invert, 0, 0, 0]
        with the neutral value where a toss failed; ``weights`` (B * C0, 2 * radius + 1) fp32, the blur taps of every field (the
        delta kernel for a field that does not blur), or ``None`` when no field blurs; ``radius``: the largest radius of the batch;
        ``call``: the noise call counter of this batch."""
        rs, C = self._rs, max(C0, 1)
        toss = rs.rand(B, 6)                  # noise, blur, gain, contrast, gamma, inverted gamma
        toss_channel = rs.rand(B, C)          # blur, per channel
        variance = rs.uniform(self.noise_variance[0], self.noise_variance[1], (B, C))
        sigma = rs.uniform(self.blur_sigma[0], self.blur_sigma[1], (B, C))
        gain = rs.uniform(self.gain[0], self.gain[1], (B, C))
        k = self._split_uniform(self.contrast, (B, C))
        gamma = self._split_uniform(self.gamma, (B, C))
        call = self._calls
        self._calls += 1
        on = lambda i, p: (toss[:, i] < p)[:, None]
        invert = on(5, self.p_gamma_invert)
        params = np.zeros((B, C, 8), dtype=np.float32)
        params[:, :, 0] = np.where(on(0, self.p_noise), np.sqrt(variance), 0.0)
        params[:, :, 1] = np.where(on(2, self.p_gain), gain, 1.0)
        params[:, :, 2] = np.where(on(3, self.p_contrast), k, 1.0)
        params[:, :, 3] = np.where(invert | on(4, self.p_gamma), gamma, 1.0)
        params[:, :, 4] = np.where(invert, 1.0, 0.0)
        params = params[:, :C0].reshape(B * C0, 8)
        blur = (on(1, self.p_blur) & (toss_channel < self.p_blur_channel))[:, :C0].reshape(-1)
        weights, radius = None, 0
        if blur.any():
            sig = sigma[:, :C0].reshape(-1)
            radius = max(int(4.0 * s + 0.5) for s in sig[blur])
            weights = np.zeros((B * C0, 2 * radius + 1), dtype=np.float32)
            weights[:, radius] = 1.0
            for f in np.nonzero(blur)[0]:
                weights[f] = gaussian_weights(sig[f], radius)
        return {"params": params, "weights": weights, "radius": radius, "call": call}

    def __call__(self, batch):
        images = batch.get(KEY_IMAGES, [])
        _require_intensity_input(images)
        B, C0 = int(images.shape[0]), int(images.shape[1])
        draws = self.draw(B, C0)
        out = dict(batch)
        out[KEY_IMAGES] = _intensity_launch(images, draws["params"], draws["weights"], self._seed, draws["call"])
        return out


def _require_intensity_input(images):
    if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.float32 and images.dim() == 5):
        raise RuntimeError("IntensityAugment (stroke_prediction_amd) works on (B, C, Z, Y, X) CUDA fp32 images: the transform is a set of "
                           "HIP kernels; there is no CPU path")


def _intensity_launch(images, params, weights, seed, call):
    """The launches of ``IntensityAugment`` on ``images`` ((B, C0, Z, Y, X) CUDA fp32) with a host table ``params`` (B * C0, 8) and host
    blur ``weights`` (B * C0, 2 * radius + 1) or ``None``: one pinned upload carries both, then three blur passes (only with weights),
    the statistics and the apply launch.  Returns the new images; the input is left as it is."""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    _require_intensity_input(images)
    src = images.contiguous()
    B, C0, Z, Y, X = src.shape
    nf, per_field = B * C0, Z * Y * X
    params = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
    if params.size != nf * 8:
        raise ValueError("IntensityAugment: %d parameter words for %d fields of 8" % (params.size, nf))
    host = params
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if weights.ndim != 2 or weights.shape[0] != nf or weights.shape[1] % 2 != 1:
            raise ValueError("IntensityAugment: blur weights are (%d, 2 * radius + 1), got %r" % (nf, weights.shape))
        host = np.concatenate((params, weights.reshape(-1)))
    words = torch.from_numpy(host).pin_memory().to(src.device, non_blocking=True)
    as_i64 = lambda u: u - (1 << 64) if u >= (1 << 63) else u
    seed, call = as_i64(int(seed) & 0xFFFFFFFFFFFFFFFF), as_i64(int(call) & 0xFFFFFFFFFFFFFFFF)
    dst = torch.empty_like(src)
    if weights is not None:
        tmp = torch.empty_like(src)
        L.call("sp_blur3d_reflect_batch", O.ptr(src), O.ptr(dst), O.ptr(tmp), O.ptr(words[nf * 8:]), nf, Z, Y, X, (weights.shape[1] - 1) // 2,
               O.stream())
        src = dst
    partials = torch.empty((nf, 64, 4), dtype=torch.float32, device=src.device)
    L.call("sp_intensity_stats_partials", O.ptr(src), O.ptr(words), O.ptr(partials), nf, per_field, seed, call, O.stream())
    L.call("sp_intensity_apply_batch", O.ptr(src), O.ptr(dst), O.ptr(words), O.ptr(partials), nf, per_field, seed, call, O.stream())
    return dst


_CHAIN_ORDER = ("ResamplePlaneXY", "flip", "PadImages", "RandomPatch", "ToTensor")


def _parse_chain(transforms):
    """A script's transform list -> {stage: transform}: [ResamplePlaneXY] [HemisphericFlipFixedToCaseId | HemisphericFlip] [PadImages]
    [RandomPatch] ToTensor, in this order.  Anything else -- the per-sample ``ElasticDeform`` included -- is a ``ValueError``."""
    stages, last = {}, -1
    for t in transforms:
        if isinstance(t, ResamplePlaneXY):
            stage = 0
        elif isinstance(t, (HemisphericFlipFixedToCaseId, HemisphericFlip)):
            stage = 1
        elif isinstance(t, PadImages):
            stage = 2
        elif isinstance(t, RandomPatch):
            stage = 3
        elif isinstance(t, ToTensor):
            stage = 4
        else:
            raise ValueError("CachedBatchLoader: %s cannot run from the device cache (the gather does ResamplePlaneXY, HemisphericFlip"
                             "[FixedToCaseId], PadImages, RandomPatch, ToTensor); hand a batch-level transform such as BatchElasticDeform to "
                             "batch_transform= instead" % type(t).__name__)
        if stage <= last:
            raise ValueError("CachedBatchLoader: %s out of order; the chain is [ResamplePlaneXY] [HemisphericFlipFixedToCaseId | "
                             "HemisphericFlip] [PadImages] [RandomPatch] ToTensor" % type(t).__name__)
        stages[_CHAIN_ORDER[stage]] = t
        last = stage
    if last != 4:
        raise ValueError("CachedBatchLoader: the chain must end in ToTensor")
    return stages


class CachedBatchLoader(object):
    """The loader of ``_loader`` over a ``DeviceCaseCache``: the same index order (``SubsetRandomSampler`` + ``BatchSampler``,
    ``drop_last=False``), the same batch dict (keys, dtypes, shapes, devices) as the collated batch of the per-sample chain
    ``transforms``, built per batch by one pinned upload of the (B, 5) table, one ``sp_patch_gather_batch`` launch and one
    ``index_select`` for ``clinical``; ``batch_transform`` is applied afterwards.  With ``patch_augment`` (a ``PatchAugment``) the launch
    is ``sp_patch_sample_batch`` and the upload also carries its transforms; the batch dict is the same.  Random draws come from Python's ``random``, per
    sample in the chain's order (``random.random()`` of ``HemisphericFlip``, then ``randint`` for x, y, z of ``RandomPatch``): with
    equal ``random`` state a batch equals the per-sample chain on the same cases bit for bit.  ``ResamplePlaneXY`` was applied
    when the cache was filled.  ``last_table``: the host copy of the latest batch's table, as drawn; ``last_table_device``: the device
    table the gather read (reading it synchronises with the stream).

    ``foreground`` (a ``ForegroundOversample``): the uniform origins are drawn as always -- the ``random`` stream is the same with and
    without it, and they are the fallback of a case without foreground -- its draws ride in the upload that carries the table, and
    ``sp_patch_origins_fg`` rewrites the origins of the forced samples on the device between the upload and the gather: two launches
    per batch instead of one, no host read, no synchronisation.  It needs a ``RandomPatch`` in the chain, labels in the cache and a
    patch crop no larger than the image padding on every axis (only then does a clamped origin keep the picked voxel inside the
    label patch).  With a ``patch_augment`` the picked voxel sits at its drawn position before the transform, so the share of
    patches with foreground is a statistical property there, not a per-sample guarantee."""

    def __init__(self, cache, items, batch_size, transforms, batch_transform=None, patch_augment=None, foreground=None):
        from torch.utils.data.sampler import BatchSampler, SubsetRandomSampler
        self._stages = _parse_chain(transforms)
        missing = [i for i in items if i not in cache.slot_of]
        if missing:
            raise ValueError("CachedBatchLoader: items %r are not in the cache" % (missing,))
        self.cache, self.dataset, self.batch_size, self.batch_transform = cache, cache.dataset, batch_size, batch_transform
        self.patch_augment = patch_augment
        self.sampler = SubsetRandomSampler(items)
        self.batch_sampler = BatchSampler(self.sampler, batch_size, drop_last=False)
        self.foreground = foreground
        self.last_table = self.last_table_device = None
        Z, Y, X = cache.shape_zyx
        pad, patch = self._stages.get("PadImages"), self._stages.get("RandomPatch")
        self._pad0 = (pad._padx, pad._pady, pad._padz) if pad is not None else (0, 0, 0)
        self._padval0 = pad._pad_value if pad is not None else 0.0
        self._padded = (X + 2 * self._pad0[0], Y + 2 * self._pad0[1], Z + 2 * self._pad0[2])      # what RandomPatch sees
        if patch is not None:
            self._ext0 = (patch._w, patch._h, patch._d)
            self._ext1 = (patch._w - 2 * patch._padx, patch._h - 2 * patch._pady, patch._d - 2 * patch._padz)
        else:
            self._ext0, self._ext1 = self._padded, (X, Y, Z)
        self._omax = tuple(n - e for n, e in zip(self._padded, self._ext0))
        if foreground is not None:
            if patch is None:
                raise ValueError("CachedBatchLoader: foreground oversampling moves the origin of a RandomPatch; the chain has none")
            if cache.labels is None:
                raise ValueError("CachedBatchLoader: foreground oversampling reads the cached labels; the cache holds none")
            _chanmask(foreground.channels, int(cache.labels.shape[1]), "CachedBatchLoader(foreground=...)")
            crop = (patch._padx, patch._pady, patch._padz)
            if any(c > p for c, p in zip(crop, self._pad0)):
                raise ValueError("CachedBatchLoader: foreground oversampling needs RandomPatch's pad %r <= PadImages' pad %r on every axis: "
                                 "only then does a clamped origin keep the picked voxel inside the label patch" % (crop, self._pad0))

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        for items in self.batch_sampler:
            yield self.make_batch(items)

    def _row(self, item):
        slot = self.cache.slot_of[item]
        flip, patch = self._stages.get("flip"), self._stages.get("RandomPatch")
        flag = 0
        if isinstance(flip, HemisphericFlip):
            flag = int(random.random() > 0.5)
        elif flip is not None:
            flag = int(self.cache.case_ids[slot] > flip.split_id)
        origin = (0, 0, 0)
        if patch is not None:
            origin = tuple(random.randint(0, n - e) for n, e in zip(self._padded, self._ext0))
        return (slot,) + origin + (flag,)

    def make_batch(self, items):
        from torch.utils.data import default_collate
        cache = self.cache
        table = torch.tensor([self._row(int(i)) for i in items], dtype=torch.int32)
        self.last_table = table
        fg = (self.foreground, self._omax) if self.foreground is not None else ()
        if self.patch_augment is not None:
            images, labels, table_dev = _sample_launch(cache, table, self._ext0, self._pad0, self._padval0, self._ext1, (0, 0, 0),
                                                       self.patch_augment, *fg)
        else:
            images, labels, table_dev = _gather_launch(cache, table, self._ext0, self._pad0, self._padval0, self._ext1, (0, 0, 0), *fg)
        self.last_table_device = table_dev
        slots = table[:, 0].tolist()
        batch = {KEY_CASE_ID: default_collate([cache.case_ids[s] for s in slots]),
                 KEY_CLINICAL_IDX: default_collate([cache.clinical_idx[s] for s in slots]),
                 KEY_IMAGES: images, KEY_LABELS: labels,
                 KEY_GLOBAL: cache.clinical.index_select(0, table_dev[:, 0]) if cache.clinical is not None else []}
        return self.batch_transform(batch) if self.batch_transform is not None else batch


def _cache_prefix(chains):
    """the ``ResamplePlaneXY`` steps the chains start with -- they must agree, since the loaders share one cache"""
    found = [_parse_chain(c).get("ResamplePlaneXY") for c in chains]
    keys = set((t._scale_factor, t._order) if t is not None else None for t in found)
    if len(keys) != 1:
        raise ValueError("device_cache: the training and the validation chain resample differently (%r); they share one cache" % (keys,))
    return [found[0]] if found[0] is not None else []


def _cached_loaders(modalities, labels, chains, item_lists, batch_size, batch_transforms, patch_augments=None, foregrounds=None):
    if not torch.cuda.is_available():
        raise RuntimeError("device_cache=True (stroke_prediction_amd) needs a GPU: the case cache lives in device memory and the "
                           "batches are gathered by a HIP kernel; there is no CPU path")
    ds = _dataset(modalities, labels, _cache_prefix(chains), "cuda")
    cache = DeviceCaseCache(ds, "cuda", items=[i for items in item_lists for i in items])
    patch_augments = patch_augments or [None] * len(chains)
    foregrounds = foregrounds or [None] * len(chains)
    return [CachedBatchLoader(cache, items, batch_size, chain, bt, pa, fg)
            for chain, items, bt, pa, fg in zip(chains, item_lists, batch_transforms, patch_augments, foregrounds)]


def _check_patch_augment(patch_augment, device_cache):
    if patch_augment is not None and not device_cache:
        raise ValueError("patch_augment needs device_cache=True: the patches are sampled from the device-resident case cache "
                         "(sp_patch_sample_batch); the per-sample chain has no such path")


def _check_foreground(foreground, device_cache):
    if foreground is not None and not device_cache:
        raise ValueError("foreground needs device_cache=True: the foreground voxel is picked from the labels of the device-resident case "
                         "cache (sp_patch_origins_fg); the per-sample chain has no such path")


def split_data_loader3D(modalities, labels, indices, batch_size, random_seed=None, valid_size=0.5, shuffle=True,
                        num_workers=4, pin_memory=False, train_transform=[], valid_transform=[], batch_transform=None,
                        device_cache=False, patch_augment=None, foreground=None):
    """data.py:113-147: one fold -> (training loader, validation loader); the first ``valid_size`` share of the
    (seed-shuffled) fold validates.  ``batch_transform`` (e.g. ``BatchElasticDeform``): applied to every collated TRAINING
    batch; the validation loader never gets it.  ``device_cache``: both loaders are ``CachedBatchLoader``s over one shared
    ``DeviceCaseCache`` (needs a GPU).  ``patch_augment`` (a ``PatchAugment``; needs ``device_cache``): the TRAINING loader samples
    its patches through it; the validation loader never gets it.  ``foreground`` (a ``ForegroundOversample``; needs ``device_cache``):
    the TRAINING loader forces its share of every batch onto foreground; the validation loader never gets it."""
    assert 0 <= valid_size <= 1, "[!] valid_size should be in the range [0, 1]."
    assert train_transform and valid_transform, "You must provide at least a numpy-to-torch transformation."
    _check_patch_augment(patch_augment, device_cache)
    _check_foreground(foreground, device_cache)
    dev = _pipeline_device()
    ds_train, ds_valid = _dataset(modalities, labels, train_transform, dev), _dataset(modalities, labels, valid_transform, dev)
    items = _fold_items(ds_train, indices, shuffle, random_seed)
    split = int(np.floor(valid_size * len(items)))
    if device_cache:
        return tuple(_cached_loaders(modalities, labels, [train_transform, valid_transform], [items[split:], items[:split]], batch_size,
                                     [batch_transform, None], [patch_augment, None], [foreground, None]))
    return (_loader(ds_train, items[split:], batch_size, num_workers, pin_memory, True, batch_transform),
            _loader(ds_valid, items[:split], batch_size, num_workers, pin_memory, False))


def single_data_loader3D(modalities, labels, indices, batch_size, random_seed=None, valid_size=0.5, shuffle=True,
                         num_workers=4, pin_memory=False, train_transform=[], batch_transform=None, device_cache=False,
                         patch_augment=None, foreground=None):
    """data.py:150-172; ``batch_transform``, ``device_cache``, ``patch_augment``, ``foreground``: as for ``split_data_loader3D``."""
    assert train_transform, "You must provide at least a numpy-to-torch transformation."
    _check_patch_augment(patch_augment, device_cache)
    _check_foreground(foreground, device_cache)
    ds = _dataset(modalities, labels, train_transform, _pipeline_device())
    items = _fold_items(ds, indices, shuffle, random_seed)
    if device_cache:
        return _cached_loaders(modalities, labels, [train_transform], [items], batch_size, [batch_transform], [patch_augment], [foreground])[0]
    return _loader(ds, items, batch_size, num_workers, pin_memory, True, batch_transform)


def get_stroke_shape_training_data(modalities, labels, train_transform, valid_transform, fold_indices, ratio, seed=4,
                                   batchsize=2, split=True, batch_transform=None, device_cache=False, patch_augment=None,
                                   foreground=None):
    """data.py:175-182 (``num_workers=0``: the transforms run in the training process -- here on its GPU)."""
    if split:
        return split_data_loader3D(modalities, labels, fold_indices, batchsize, random_seed=seed, valid_size=ratio,
                                   train_transform=train_transform, valid_transform=valid_transform, num_workers=0,
                                   batch_transform=batch_transform, device_cache=device_cache, patch_augment=patch_augment,
                                   foreground=foreground)
    return single_data_loader3D(modalities, labels, fold_indices, batchsize, random_seed=seed, valid_size=ratio,
                                train_transform=train_transform, num_workers=0, batch_transform=batch_transform,
                                device_cache=device_cache, patch_augment=patch_augment, foreground=foreground), None


get_stroke_prediction_training_data = get_stroke_shape_training_data      # data.py:185-192: the same factory


def get_testdata(modalities, labels, indices, random_seed=None, shuffle=True, num_workers=4, pin_memory=False, transform=[]):
    """data.py:195-212: batch size 1 (the case metrics are computed per batch)."""
    assert transform, "You must provide at least a numpy-to-torch transformation."
    ds = _dataset(modalities, labels, transform, _pipeline_device())
    return _loader(ds, _fold_items(ds, indices, shuffle, random_seed), 1, 0 if _pipeline_device() else num_workers, pin_memory, True)
