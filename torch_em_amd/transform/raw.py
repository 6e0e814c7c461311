"""Raw-data transforms on the hot path (reference torch_em/transform/raw.py).

Built: `standardize`, `normalize`, `normalize_percentile`, `RandomPercentileNormalization`, `RandomContrast`,
`AdditiveGaussianNoise`, `AdditivePoissonNoise`, `PoissonNoise`, `GaussianBlur`, `RawTransform`, `get_raw_transform`,
`get_default_mean_teacher_augmentations`: everything the reference's module offers.  Each dispatches on its input: a CUDA
tensor runs through the HIP kernels of csrc/rawnorm.hip and csrc/rawaug.hip (nothing is read back, so they run inside the
input pipeline's side stream and as `predict_with_halo(preprocess=...)`); numpy input takes the reference's numpy
expression.  For the deterministic transforms that is also the CPU oracle of the device path -- the two agree bit for bit
on float32 data.  A CPU torch tensor counts as numpy input and comes back as a numpy array (the reference returns a tensor
there; `GaussianBlur` returns a tensor on every path, as the reference's does): on this path tensors live on the device.

The noise transforms draw their scalar (std, lam, multiplier) with `np.random.uniform` on every path.  The noise FIELD of
the numpy branch is the reference's `np.random` draw; on the device it comes from a stream of the package's own, because
numpy's cannot be reproduced there: Philox4x32-10 keyed by one 64-bit seed per call (drawn from `np.random`, so
`np.random.seed` pins a device call), counter = (element, row, redraw).  DESIGN.md specifies the stream and both samplers;
`_philox.py` implements them in numpy, and the tests compare the device with it word for word and sample for sample.  The
two branches therefore agree in distribution, not value by value.  `GaussianBlur` is defined by torchvision in the
reference; here its arithmetic is written out (see the class), so the package needs no torchvision.
"""
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from .. import ops


def standardize(raw, mean=None, std=None, axis=None, eps: float = 1e-7, per_sample: bool = False):
    """(raw - mean) / (std + eps), the default raw transform (reference `:40-65`, `segmentation.py:394-395`).
    A CUDA tensor runs through one HIP pass pair (`tem_standardize`) with the reference's semantics: `axis=None` means
    statistics over the WHOLE array.  `per_sample=True` (not in the reference: for a device batch [N, ...] that the
    reference would have standardised sample by sample in its loader workers) or `axis` = all axes but the first give
    one mean / std per entry of the first axis.  numpy input, or explicit mean / std: the reference's numpy expression."""
    if torch.is_tensor(raw) and raw.is_cuda and mean is None and std is None:
        rest = tuple(range(1, raw.dim()))
        if axis is not None and tuple(a % raw.dim() for a in np.atleast_1d(axis)) == rest:
            per_sample, axis = True, None
        if axis is None:
            x = raw.float()
            return ops.standardize(x, eps) if per_sample else ops.standardize(x.reshape(1, -1), eps).reshape(x.shape)
        raise NotImplementedError("standardize on the device: axis must be None or all axes but the first")
    raw = np.asarray(raw, dtype="float32")
    mean = raw.mean(axis=axis, keepdims=True) if mean is None else mean
    std = raw.std(axis=axis, keepdims=True) if std is None else std
    return (raw - mean) / (std + eps)


def _on_device(raw) -> bool:
    return torch.is_tensor(raw) and raw.is_cuda


def _as_rows(raw: torch.Tensor, axis, per_sample: bool, what: str) -> torch.Tensor:
    """The device tensor as [rows, ...]: `axis` None -> one row (the whole array); a trailing run of axes -> one row per
    entry of the leading axes (per sample, per channel); per_sample -> all axes but the first."""
    nd = raw.dim()
    if per_sample:
        if axis is not None:
            raise ValueError(f"{what}: give axis or per_sample=True, not both")
        lead = min(1, nd)
    elif axis is None:
        lead = 0
    else:
        axes = sorted(int(a) % nd for a in np.atleast_1d(axis))
        lead = axes[0]
        if axes != list(range(lead, nd)):
            raise NotImplementedError(f"{what} on the device: axis must be None or a trailing run of axes (got {axis} for "
                                      f"{nd} dimensions); reduce over other axes on the host or permute the tensor first")
    n = 1
    for s in raw.shape[:lead]:
        n *= int(s)
    return raw.reshape(n, -1)


def _numpy_axis(raw, axis, per_sample: bool):
    return tuple(range(1, raw.ndim)) if per_sample and axis is None else axis


def normalize(raw, minval=None, maxval=None, axis=None, eps: float = 1e-7, per_sample: bool = False):
    """(raw - min) / (max(raw - min) + eps): into [0, 1] (reference `:88-116`).
    CUDA tensor: row min / max, coefficients and the apply run as HIP kernels; `axis` is None (whole array) or a trailing
    run of axes (one min / max per entry of the leading axes: per sample, per channel), `per_sample=True` (not in the
    reference) is all axes but the first; anything else raises NotImplementedError.  `minval` / `maxval` may be python
    numbers (both: the apply kernel alone; one: the other comes from the row min / max as in the reference).  Integer and 16-bit tensors are cast to float32 first.  The result equals the numpy
    branch on the same float32 data bit for bit.  NaN input is undefined on the device.
    numpy input: the reference's expression."""
    if _on_device(raw):
        rows = _as_rows(raw, axis, per_sample, "normalize")
        for name, v in (("minval", minval), ("maxval", maxval)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float))):
                raise NotImplementedError(f"normalize on the device: {name} must be a python number or None")
        return ops.normalize(rows, eps, minval=minval, maxval=maxval).reshape(raw.shape)
    raw = np.asarray(raw).astype("float32")   # always a copy: the steps below work in place, in float32
    axis = _numpy_axis(raw, axis, per_sample)
    np.subtract(raw, raw.min(axis=axis, keepdims=True) if minval is None else minval, out=raw)
    np.divide(raw, (raw.max(axis=axis, keepdims=True) if maxval is None else maxval) + eps, out=raw)
    return raw


def normalize_percentile(raw, lower=1.0, upper=99.0, axis=None, eps: float = 1e-7, per_sample: bool = False):
    """(raw - p_lower) / (p_upper - p_lower + eps) with `np.percentile`'s linear interpolation (reference `:119-140`).
    CUDA tensor: exact order statistics from a radix select (no sort, no read-back), numpy's float32 interpolation and the
    apply kernel; `axis` / `per_sample` as in `normalize`; `lower` / `upper` may be sequences with one entry per row.
    Integer and 16-bit tensors are cast to float32 first, so the result is the reference's for `raw.astype("float32")` --
    on integer input the reference itself interpolates the percentiles in float64 and differs from that in the last bits.
    NaN input is undefined on the device.  numpy input: the reference's expression."""
    if _on_device(raw):
        rows = _as_rows(raw, axis, per_sample, "normalize_percentile")
        return ops.normalize_percentile(rows, lower, upper, eps).reshape(raw.shape)
    raw = np.asarray(raw)
    axis = _numpy_axis(raw, axis, per_sample)
    if np.ndim(lower) or np.ndim(upper):   # one pair per entry of the first axis
        lower, upper = np.broadcast_to(lower, raw.shape[:1]), np.broadcast_to(upper, raw.shape[:1])
        return np.stack([normalize_percentile(r, float(lo), float(up), eps=eps) for r, lo, up in zip(raw, lower, upper)])
    v_lower = np.percentile(raw, lower, axis=axis, keepdims=True)
    return normalize(raw, v_lower, np.percentile(raw, upper, axis=axis, keepdims=True) - v_lower, eps=eps)


def _check_bounds(values, upper: bool):
    name = "upper_percentile_bounds" if upper else "lower_percentile_bounds"
    if not isinstance(values, (tuple, list)) or len(values) != 2:
        raise ValueError(f"{name} must contain exactly two values.")
    lo, hi = float(values[0]), float(values[1])
    ok = np.isfinite(lo) and np.isfinite(hi) and ((50.0 < lo <= hi <= 100.0) if upper else (0.0 <= lo <= hi < 50.0))
    if not ok:
        raise ValueError(f"{name} must be a finite interval within {'(50, 100]' if upper else '[0, 50)'}.")
    return lo, hi


def _uniform_kwargs(kwargs, bounds):
    if kwargs is not None:
        raise ValueError("Uniform sampling does not accept distribution_kwargs.")
    return None


def _normal_kwargs(kwargs, bounds):
    """{"mean", "std"} exactly, as floats; the mean inside the lower bounds, the width finite and not negative"""
    if not isinstance(kwargs, dict) or sorted(kwargs) != ["mean", "std"]:
        raise ValueError("Normal sampling requires exactly the distribution_kwargs 'mean' and 'std'.")
    out = {key: float(kwargs[key]) for key in ("mean", "std")}
    if not (np.isfinite(out["mean"]) and bounds[0] <= out["mean"] <= bounds[1]):
        raise ValueError("The normal distribution mean must be finite and within lower_percentile_bounds.")
    if not (np.isfinite(out["std"]) and out["std"] >= 0.0):
        raise ValueError("The normal distribution std must be finite and non-negative.")
    return out


_SAMPLERS = {"uniform": _uniform_kwargs, "normal": _normal_kwargs}


def _check_seed(seed):
    if seed is None:
        return None
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):   # True is an int, and is not a seed
        raise TypeError("seed must be an integer or None.")
    if seed < 0:
        raise ValueError("seed must be non-negative.")
    return int(seed)


class RandomPercentileNormalization:
    """Percentile normalisation with randomly drawn percentiles, output clipped to [0, 1] (reference `:143-297`; same
    arguments, validation, seeding and draws).  `lower` is drawn from `lower_percentile_bounds`, `upper` from
    `upper_percentile_bounds` (default: the lower bounds mirrored around 50), uniformly or -- `distribution="normal"`,
    `distribution_kwargs={"mean": m, "std": s}` -- from a normal distribution (the upper one mirrored) clipped to the bounds,
    rounded to `rounding_decimals`.  `seed`: a private generator per DataLoader worker, else numpy's global state.
    `per_sample=True` (not in the reference): one pair per entry of the first axis, drawn in order from the same generator,
    percentiles over all other axes -- a batch then equals the reference called sample by sample."""

    def __init__(self, lower_percentile_bounds: Tuple[float, float] = (0.0, 5.0),
                 upper_percentile_bounds: Optional[Tuple[float, float]] = None, distribution: str = "uniform",
                 distribution_kwargs: Optional[Dict[str, float]] = None, rounding_decimals: Optional[int] = 1, axis=None,
                 seed: Optional[int] = None, eps: float = 1e-7, per_sample: bool = False):
        lower_percentile_bounds = _check_bounds(lower_percentile_bounds, upper=False)
        if upper_percentile_bounds is None:
            upper_percentile_bounds = (100.0 - lower_percentile_bounds[1], 100.0 - lower_percentile_bounds[0])
        upper_percentile_bounds = _check_bounds(upper_percentile_bounds, upper=True)
        if distribution not in _SAMPLERS:
            raise ValueError("distribution must be 'uniform' or 'normal'.")
        distribution_kwargs = _SAMPLERS[distribution](distribution_kwargs, lower_percentile_bounds)
        decimals_ok = rounding_decimals is None or (type(rounding_decimals) is int and rounding_decimals >= 0)
        if not decimals_ok:
            raise ValueError("rounding_decimals must be a non-negative integer or None.")
        if not np.isfinite(eps) or eps <= 0.0:
            raise ValueError("eps must be finite and greater than zero.")
        seed = _check_seed(seed)
        if per_sample and axis is not None:
            raise ValueError("give axis or per_sample=True, not both")
        self.lower_percentile_bounds = lower_percentile_bounds
        self.upper_percentile_bounds = upper_percentile_bounds
        self.distribution = distribution
        self.distribution_kwargs = distribution_kwargs
        self.rounding_decimals = rounding_decimals
        self.axis = axis
        self.seed = seed
        self.eps = float(eps)
        self.per_sample = bool(per_sample)
        self._random_generator = None
        self._random_generator_worker_id = None

    def _generator(self):
        if self.seed is None:
            return np.random
        info = torch.utils.data.get_worker_info()
        worker = None if info is None else info.id
        if self._random_generator is None or self._random_generator_worker_id != worker:
            self._random_generator = np.random.default_rng(np.random.SeedSequence([self.seed, worker or 0]))
            self._random_generator_worker_id = worker
        return self._random_generator

    def _rounded(self, value) -> float:
        return float(value) if self.rounding_decimals is None else round(float(value), self.rounding_decimals)

    def sample_percentiles(self) -> Tuple[float, float]:
        """Draw one valid (lower, upper) percentile pair."""
        rng = self._generator()
        if self.distribution == "uniform":
            lower = rng.uniform(*self.lower_percentile_bounds)
            upper = rng.uniform(*self.upper_percentile_bounds)
        else:
            def draw(mean, std):   # a zero width draws nothing from the generator
                return rng.normal(mean, std) if std != 0.0 else mean
            lower = draw(**self.distribution_kwargs)
            upper = 100.0 - draw(**self.distribution_kwargs)   # the lower distribution mirrored around 50
        # the tails of the normal distribution may leave the bounds
        return (float(np.clip(self._rounded(lower), *self.lower_percentile_bounds)),
                float(np.clip(self._rounded(upper), *self.upper_percentile_bounds)))

    def __call__(self, raw):
        if self.per_sample:
            pairs = [self.sample_percentiles() for _ in range(len(raw))]
            lower, upper = [p[0] for p in pairs], [p[1] for p in pairs]
        else:
            lower, upper = self.sample_percentiles()
        if _on_device(raw):
            rows = _as_rows(raw, self.axis, self.per_sample, "RandomPercentileNormalization")
            return ops.normalize_percentile(rows, lower, upper, self.eps, clip=(0.0, 1.0)).reshape(raw.shape)
        out = normalize_percentile(raw, lower, upper, axis=self.axis, eps=self.eps, per_sample=self.per_sample)
        return np.clip(out, 0.0, 1.0)


class RandomContrast:
    """mean + alpha * (img - mean) with alpha drawn uniformly from `alpha` by `np.random.uniform`, then clipped with
    `clip_kwargs` (reference `:305-334`).  A CUDA tensor runs through the contrast kernel in float32 (multiply and add are
    rounded separately, as numpy does); `per_sample=True` (not in the reference) draws one alpha per entry of the first
    axis, in order.  On the device `clip_kwargs` may hold `a_min` and `a_max` only (None: that side stays open); any other
    np.clip keyword raises."""

    def __init__(self, alpha: Tuple[float, float] = (0.5, 2), mean: float = 0.5,
                 clip_kwargs: Optional[Dict] = {"a_min": 0, "a_max": 1}, per_sample: bool = False):
        self.alpha = alpha
        self.mean = mean
        self.clip_kwargs = clip_kwargs
        self.per_sample = bool(per_sample)

    def __call__(self, img):
        n = len(img) if self.per_sample else 1
        alpha = [np.random.uniform(self.alpha[0], self.alpha[1]) for _ in range(n)]
        if _on_device(img):
            clip = None
            if self.clip_kwargs:
                unknown = set(self.clip_kwargs) - {"a_min", "a_max"}
                if unknown:
                    raise ValueError(f"RandomContrast on the device: clip_kwargs takes a_min and a_max only, got {sorted(unknown)}")
                clip = (self.clip_kwargs.get("a_min"), self.clip_kwargs.get("a_max"))
            rows = img.reshape(n, -1)
            return ops.contrast(rows, alpha, self.mean, clip).reshape(img.shape)
        img = np.asarray(img)
        if self.per_sample:
            res = np.stack([self.mean + a * (r - self.mean) for a, r in zip(alpha, img)])
        else:
            res = self.mean + alpha[0] * (img - self.mean)
        return np.clip(res, **self.clip_kwargs) if self.clip_kwargs else res


def _device_clip(clip_kwargs, who: str):
    """clip_kwargs -> (a_min, a_max) or None, by RandomContrast's rule for the device"""
    if not clip_kwargs:
        return None
    unknown = set(clip_kwargs) - {"a_min", "a_max"}
    if unknown:
        raise ValueError(f"{who} on the device: clip_kwargs takes a_min and a_max only, got {sorted(unknown)}")
    return (clip_kwargs.get("a_min"), clip_kwargs.get("a_max"))


def _field_seed() -> int:
    """the 64-bit seed of one device noise field, from numpy's global state (so np.random.seed pins a device call)"""
    return int(np.random.randint(0, 2 ** 63, dtype=np.int64))


class AdditiveGaussianNoise:
    """img + N(0, std) with std drawn uniformly from `scale` by `np.random.uniform` (reference `:337-363`).  As in the
    reference a truthy `clip_kwargs` clips to [0, 1] whatever it holds.
    numpy input: the reference's expression and `np.random.normal` draw.  A CUDA tensor: std is drawn the same way, then one
    64-bit seed by `np.random.randint(0, 2**63, dtype=np.int64)`, and the Gauss kernel adds std * z with z from the package's
    counter-based stream (`_philox.py`; not numpy's stream, which has no device counterpart) -- `np.random.seed` makes the
    call reproducible.  `per_sample=True` (not in the reference): one std per entry of the first axis, drawn in order, and
    still one seed (each sample is its own row of the stream); on numpy input it is the reference sample by sample.  On the
    device `clip_kwargs` may hold `a_min` and `a_max` only; any other np.clip keyword raises."""

    def __init__(self, scale: Tuple[float, float] = (0.0, 0.3), clip_kwargs: Optional[Dict] = {"a_min": 0, "a_max": 1},
                 per_sample: bool = False):
        self.scale = scale
        self.clip_kwargs = clip_kwargs
        self.per_sample = bool(per_sample)

    def _numpy(self, img):
        std = np.random.uniform(self.scale[0], self.scale[1])
        gaussian_noise = np.random.normal(0, std, size=img.shape)
        if self.clip_kwargs:
            return np.clip(img + gaussian_noise, 0, 1)
        return img + gaussian_noise

    def __call__(self, img):
        if _on_device(img):
            n = len(img) if self.per_sample else 1
            std = [np.random.uniform(self.scale[0], self.scale[1]) for _ in range(n)]
            seed = _field_seed()
            clip = (0.0, 1.0) if _device_clip(self.clip_kwargs, "AdditiveGaussianNoise") else None
            return ops.gauss_noise(img.reshape(n, -1), std, seed, clip).reshape(img.shape)
        img = np.asarray(img)
        return np.stack([self._numpy(s) for s in img]) if self.per_sample else self._numpy(img)


class AdditivePoissonNoise:
    """img + Poisson(lam) / lam with lam drawn uniformly from `lam` by `np.random.uniform` (reference `:366-391`); a truthy
    `clip_kwargs` clips to [0, 1] whatever it holds.  Dispatch, seed, `per_sample` and the device's `clip_kwargs` rule as in
    `AdditiveGaussianNoise`; the device counts come from the package's stream (inversion below lam = 10, transformed
    rejection from there).  A drawn lam == 0 raises ValueError on the device path (the reference divides by zero there)."""

    def __init__(self, lam: Tuple[float, float] = (0.0, 0.1), clip_kwargs: Optional[Dict] = {"a_min": 0, "a_max": 1},
                 per_sample: bool = False):
        self.lam = lam
        self.clip_kwargs = clip_kwargs
        self.per_sample = bool(per_sample)

    def _numpy(self, img):
        lam = np.random.uniform(self.lam[0], self.lam[1])
        poisson_noise = np.random.poisson(lam, size=img.shape) / lam
        if self.clip_kwargs:
            return np.clip(img + poisson_noise, 0, 1)
        return img + poisson_noise

    def __call__(self, img):
        if _on_device(img):
            n = len(img) if self.per_sample else 1
            lam = [np.random.uniform(self.lam[0], self.lam[1]) for _ in range(n)]
            seed = _field_seed()
            if any(np.float32(v) == 0 for v in lam):
                raise ValueError("AdditivePoissonNoise: the drawn lam is 0, and the noise is Poisson(lam) / lam")
            clip = (0.0, 1.0) if _device_clip(self.clip_kwargs, "AdditivePoissonNoise") else None
            return ops.poisson_add(img.reshape(n, -1), lam, seed, clip).reshape(img.shape)
        img = np.asarray(img)
        return np.stack([self._numpy(s) for s in img]) if self.per_sample else self._numpy(img)


class PoissonNoise:
    """Poisson((img - min) * multiplier) / multiplier + min, the multiplier drawn uniformly from `multiplier` by
    `np.random.uniform`, then np.clip with `clip_kwargs` (reference `:394-425`).  Dispatch, seed and the device's
    `clip_kwargs` rule as in `AdditiveGaussianNoise`; on the device the minimum comes from the row min / max kernel and the
    means (img - min) * multiplier must stay below 2^24.  `per_sample=True` (not in the reference): one multiplier and one
    minimum per entry of the first axis.  NaN input is undefined on the device."""

    def __init__(self, multiplier: Tuple[float, float] = (5.0, 10.0), clip_kwargs: Optional[Dict] = {"a_min": 0, "a_max": 1},
                 per_sample: bool = False):
        self.multiplier = multiplier
        self.clip_kwargs = clip_kwargs
        self.per_sample = bool(per_sample)

    def _numpy(self, img):
        multiplier = np.random.uniform(self.multiplier[0], self.multiplier[1])
        offset = img.min()
        poisson_noise = np.random.poisson((img - offset) * multiplier)
        poisson_noise = poisson_noise / multiplier + offset
        if self.clip_kwargs:
            return np.clip(poisson_noise, **self.clip_kwargs)
        return poisson_noise

    def __call__(self, img):
        if _on_device(img):
            n = len(img) if self.per_sample else 1
            mult = [np.random.uniform(self.multiplier[0], self.multiplier[1]) for _ in range(n)]
            seed = _field_seed()
            clip = _device_clip(self.clip_kwargs, "PoissonNoise")
            return ops.poisson_scaled(img.reshape(n, -1), mult, seed, clip).reshape(img.shape)
        img = np.asarray(img)
        return np.stack([self._numpy(s) for s in img]) if self.per_sample else self._numpy(img)


def gaussian_weights(sigma: float) -> torch.Tensor:
    """The normalised 1-D Gaussian of `GaussianBlur`, float32 on the CPU: kernel_size = int(2 * ceil(3 sigma) + 1) taps at
    x = linspace(-(k-1)/2, (k-1)/2, k), pdf = exp(-0.5 (x / sigma)^2), w = pdf / pdf.sum() -- torch float32 operations."""
    if not sigma > 0:
        raise ValueError(f"GaussianBlur: sigma must be positive, got {sigma}")
    k = int(2 * np.ceil(3 * sigma) + 1)
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


class GaussianBlur:
    """Gaussian blur of the last two axes with sigma drawn by `np.random.uniform(sigma[1], sigma[0])` -- the bounds swapped,
    as in the reference (`:428-454`), which hands the image to torchvision's `GaussianBlur(kernel_size, sigma)`.
    torchvision is not a dependency of this package and is not installed where its golden files are made, so the
    definition is pinned by this text and not by a golden file: the weights of `gaussian_weights` (one vector for both
    axes), their outer product, reflect padding (index -j -> j, no edge repeat) and a depth-wise 2-D convolution.  All axes
    but the last two are independent planes (a [C, D, H, W] volume is blurred in-plane only, which is what the reference
    does); the input has at least two axes and kernel_size // 2 must be smaller than both of the last two.
    numpy input or a CPU tensor: `F.pad(mode="reflect")` + `F.conv2d(groups=planes)` on the CPU; returns a torch tensor, as
    the reference does (integer input comes back as float32).  A CUDA tensor: the blur kernel (kernel_size <= 63), which
    forms the two 1-D sums one after the other and agrees with the CPU branch to rounding.  Both branches call
    `torch.empty(1).uniform_(sigma, sigma)` once, as torchvision's transform does, which keeps torch's generator in step."""

    def __init__(self, sigma: Tuple[float, float] = (0.0, 3.0)):
        self.sigma = sigma

    def __call__(self, img):
        sigma = np.random.uniform(self.sigma[1], self.sigma[0])
        w = gaussian_weights(sigma)
        torch.empty(1).uniform_(sigma, sigma)
        if _on_device(img):
            if img.dim() < 2:
                raise ValueError("GaussianBlur: the input needs at least two axes")
            return ops.blur2d(img, w.tolist()).reshape(img.shape)
        if not torch.is_tensor(img):
            img = torch.from_numpy(np.ascontiguousarray(img))
        if img.dim() < 2:
            raise ValueError("GaussianBlur: the input needs at least two axes")
        x = img if img.is_floating_point() else img.float()
        H, W = x.shape[-2:]
        pad = len(w) // 2
        if pad >= H or pad >= W:
            raise ValueError(f"GaussianBlur: the reflect border needs kernel_size // 2 < size on each axis "
                             f"({len(w)} taps on a {H} x {W} plane)")
        planes = x.reshape(1, -1, H, W)
        w = w.to(x.dtype)
        kernel = torch.mm(w[:, None], w[None, :]).expand(planes.shape[1], 1, len(w), len(w))
        out = torch.nn.functional.conv2d(torch.nn.functional.pad(planes, [pad, pad, pad, pad], mode="reflect"), kernel,
                                         groups=planes.shape[1])
        return out.reshape(x.shape)


class _Compose:
    """call the transforms in order (torchvision.transforms.Compose)"""

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img


class _RandomApply:
    """apply the transforms with probability p: skipped when p < torch.rand(1) (torchvision.transforms.RandomApply)"""

    def __init__(self, transforms, p: float = 0.5):
        self.transforms = transforms
        self.p = p

    def __call__(self, img):
        if self.p < torch.rand(1):
            return img
        for t in self.transforms:
            img = t(img)
        return img


class RawTransform:
    """The raw transform of training: `augmentation1`, then `normalizer`, then `augmentation2` (reference `:461-492`)."""

    def __init__(self, normalizer: Callable, augmentation1: Optional[Callable] = None, augmentation2: Optional[Callable] = None):
        self.normalizer = normalizer
        self.augmentation1 = augmentation1
        self.augmentation2 = augmentation2

    def __call__(self, raw):
        for step in (self.augmentation1, self.normalizer, self.augmentation2):
            if step is not None:
                raw = step(raw)
        return raw


def get_raw_transform(normalizer: Callable = standardize, augmentation1: Optional[Callable] = None,
                      augmentation2: Optional[Callable] = None) -> Callable:
    """`RawTransform(normalizer, augmentation1, augmentation2)` (reference `:495-510`)."""
    return RawTransform(normalizer, augmentation1=augmentation1, augmentation2=augmentation2)


def get_default_mean_teacher_augmentations(p: float = 0.3, norm: Optional[Callable] = None, blur_kwargs: Optional[Dict] = None,
                                           poisson_kwargs: Optional[Dict] = None, gaussian_kwargs: Optional[Dict] = None) -> Callable:
    """The default augmentations of mean-teacher training (reference `:513-546`), designed for values in [0, 1]: `norm`
    (default `normalize`), then blur with probability p, Poisson noise and additive Gaussian noise with p / 2 each; then
    `norm` again as the normaliser, then contrast with probability p.  The coin flips are `torch.rand(1)` as in
    torchvision's `RandomApply`, so `torch.manual_seed` and `np.random.seed` together pin a call."""
    if norm is None:
        norm = normalize
    aug1 = _Compose([
        norm,
        _RandomApply([GaussianBlur(**({} if blur_kwargs is None else blur_kwargs))], p=p),
        _RandomApply([PoissonNoise(**({} if poisson_kwargs is None else poisson_kwargs))], p=p / 2),
        _RandomApply([AdditiveGaussianNoise(**({} if gaussian_kwargs is None else gaussian_kwargs))], p=p / 2),
    ])
    aug2 = _RandomApply([RandomContrast(clip_kwargs={"a_min": 0, "a_max": 1})], p=p)
    return get_raw_transform(normalizer=norm, augmentation1=aug1, augmentation2=aug2)
