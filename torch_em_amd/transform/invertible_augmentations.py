"""Invertible augmentations on the device (reference torch_em/transform/invertible_augmentations.py).

The self-training trainers `*WithInvertibleAugmentations` and `UniMatchv2Trainer` take ONE raw batch from the loader, augment
it on the device -- intensity changes, then flips and rotations by multiples of 90 degrees drawn per sample -- and map
pseudo labels, label filter and student prediction back into the common frame before the loss.  Names and signatures are the
reference's: `DEFAULT_WEAK_AUGMENTATIONS`, `DEFAULT_STRONG_AUGMENTATIONS`, `get_intensity_augmentations`,
`get_geometrical_augmentations`, `get_default_augmentations`, `AugmentationSequential3D`, `InvertibleAugmenter`
(`reset` / `transform` / `reverse_transform`), `MeanTeacherAugmenters`, `FixMatchAugmenters`, `UniMatchv2Augmenters`.

The reference builds them on kornia.  kornia is not a dependency of this package (as in `transform/augmentation.py`): the
classes below carry kornia's names and arguments and are this package's own.  THE RANDOM STREAMS ARE THIS PACKAGE'S, NOT
KORNIA'S: per-sample coin flips, rotation counts and sigmas come from the torch CPU generator in the order documented on
each class (`torch.manual_seed` pins them), noise seeds from numpy's global state (`transform/raw.py`'s `_field_seed`
convention), the noise itself from the package's counter-based stream.  Nothing here reproduces kornia draw for draw.

What runs differently from the reference:
  * the whole geometric chain of a container composes, per sample, to ONE element of the dihedral group D4, and `transform`
    is one `ops.dihedral` launch (csrc/invaug.hip), `reverse_transform` another -- in 2-D and in 3-D, where depth folds into
    the planes as in the reference's `AugmentationSequential3D`.  The reference warps sample by sample;
  * the inverse is exact to the bit and differentiable (its backward pass is the forward launch with the inverse codes);
  * a draw that transposes (an odd rotation count) on a non-square patch raises ValueError -- the samples of one batch must
    share a shape; restrict `RandomRotation90` to `times=(0, 0)` or `(2, 2)` for such patches;
  * blur and noise run on `ops.blur2d` / `ops.gauss_noise`; a sample that loses its coin flip passes through bit for bit.

Drawn parameters live in `_params` of every class and of the container (a list, one entry per augmentation) and can be
passed back in (`params=`) to replay a recorded draw.
"""
from typing import Callable, Optional, Sequence

import torch

from .. import ops
from .augmentation import RandomHorizontalFlip, RandomVerticalFlip, _RandomFlip
from .raw import _field_seed

DEFAULT_WEAK_AUGMENTATIONS = {
    "intensity": {},
    "geometrical": {
        "RandomHorizontalFlip": {},
        "RandomVerticalFlip": {},
        "RandomRotation90": {"times": (-1, 2)},
    }
}

DEFAULT_STRONG_AUGMENTATIONS = {
    "intensity": {
        "RandomGaussianBlur": {"kernel_size": (3, 3), "sigma": (0.1, 1.0)},
        "RandomGaussianNoise": {"mean": (0.0), "std": (0.1)},
    },
    "geometrical": {
        "RandomHorizontalFlip": {},
        "RandomVerticalFlip": {},
        "RandomRotation90": {"times": (-1, 2)},
    }
}


def _coin(n: int, p: float, same_on_batch: bool) -> torch.Tensor:
    """one draw of torch.rand per sample (one in all with same_on_batch), as `_RandomFlip.generate_parameters`"""
    if same_on_batch:
        return (torch.rand(1) < p).expand(n).clone()
    return torch.rand(n) < p


class RandomRotation90(torch.nn.Module):
    """Rotation of the last two axes by `times` * 90 degrees with probability p per sample (kornia's `RandomRotation90`):
    `times` is drawn uniformly from the CLOSED integer range `times=(lo, hi)` and has `torch.rot90`'s sign convention
    (positive: from the H axis towards the W axis).  Draws, in this order: `torch.rand(n) < p`, then
    `torch.randint(lo, hi + 1, (n,))`."""
    spatial = 2

    def __init__(self, times=(-1, 2), p: float = 0.5, same_on_batch: bool = False, keepdim: bool = False):
        super().__init__()
        times = tuple(int(t) for t in times)
        if len(times) != 2 or times[0] > times[1]:
            raise ValueError(f"RandomRotation90: times must be a (min, max) pair of integers, got {times}")
        self.times, self.p, self.same_on_batch, self.keepdim = times, p, same_on_batch, keepdim
        self._params = None

    def generate_parameters(self, batch_shape):
        n = batch_shape[0]
        prob = _coin(n, self.p, self.same_on_batch)
        m = 1 if self.same_on_batch else n
        times = torch.randint(self.times[0], self.times[1] + 1, (m,)).expand(n).clone()
        return {"batch_prob": prob, "times": times}

    def forward(self, input: torch.Tensor, params=None) -> torch.Tensor:
        return AugmentationSequential(self)(input, params=None if params is None else [params])

    def inverse(self, input: torch.Tensor, params=None) -> torch.Tensor:
        return AugmentationSequential(self).inverse(input, params=[self._params if params is None else params])


def _gauss_taps(ksize: int, sigma: float):
    """kornia's 1-D Gaussian of a FIXED tap count: exp(-x^2 / (2 sigma^2)) at x = -(k // 2) .. k // 2, normalised (float32)"""
    x = torch.arange(ksize, dtype=torch.float32) - ksize // 2
    g = torch.exp(-x.pow(2.0) / (2 * float(sigma) ** 2))
    return (g / g.sum()).tolist()


class RandomGaussianBlur(torch.nn.Module):
    """Gaussian blur of the last two axes with `kernel_size = (ky, kx)` taps (odd) and a sigma drawn uniformly from
    `sigma=(lo, hi)` per sample, applied with probability p per sample; reflect border (kornia's `RandomGaussianBlur`).
    Draws, in this order: `torch.rand(n) < p`, then `torch.rand(n)` scaled to the sigma range.  Runs `ops.blur2d` once per
    sample that won its coin flip (each has its own weights); the others keep their bits.  float32."""

    def __init__(self, kernel_size, sigma, border_type: str = "reflect", p: float = 0.5, same_on_batch: bool = False,
                 keepdim: bool = False):
        super().__init__()
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(int(k) for k in kernel_size)
        if len(ks) != 2 or any(k < 1 or k % 2 == 0 for k in ks):
            raise ValueError(f"RandomGaussianBlur: kernel_size must be odd and positive, got {kernel_size}")
        sg = (float(sigma), float(sigma)) if isinstance(sigma, (int, float)) else tuple(float(s) for s in sigma)
        if len(sg) != 2 or not 0 < sg[0] <= sg[1]:
            raise ValueError(f"RandomGaussianBlur: sigma must be a positive (min, max) pair, got {sigma}")
        if border_type != "reflect":
            raise NotImplementedError("RandomGaussianBlur: the blur kernel has the reflect border only")
        self.kernel_size, self.sigma, self.p, self.same_on_batch, self.keepdim = ks, sg, p, same_on_batch, keepdim
        self._params = None

    def generate_parameters(self, batch_shape):
        n = batch_shape[0]
        prob = _coin(n, self.p, self.same_on_batch)
        m = 1 if self.same_on_batch else n
        sigma = (torch.rand(m, dtype=torch.float64) * (self.sigma[1] - self.sigma[0]) + self.sigma[0]).expand(n).clone()
        return {"batch_prob": prob, "sigma": sigma}

    def forward(self, input: torch.Tensor, params=None) -> torch.Tensor:
        params = self.generate_parameters(input.shape) if params is None else params
        self._params = params
        if input.dtype != torch.float32:
            raise ValueError(f"RandomGaussianBlur: expected a float32 tensor, got {input.dtype}")
        win = [n for n in range(input.shape[0]) if bool(params["batch_prob"][n])]
        if not win:
            return input
        out = input.clone()
        for n in win:
            s = float(params["sigma"][n])
            out[n] = ops.blur2d(input[n], _gauss_taps(self.kernel_size[0], s), _gauss_taps(self.kernel_size[1], s))
        return out


class RandomGaussianNoise(torch.nn.Module):
    """x + mean + std * z, z standard normal, with probability p per sample (kornia's `RandomGaussianNoise`).  Draws:
    `torch.rand(n) < p` from the torch CPU generator, then one 64-bit seed from numpy's global state (`_field_seed`,
    transform/raw.py); z comes from the package's counter-based stream, row k of it for the k-th sample that won its coin
    flip.  One `ops.gauss_noise` launch over those samples; the others keep their bits.  float32."""

    def __init__(self, mean: float = 0.0, std: float = 1.0, p: float = 0.5, same_on_batch: bool = False, keepdim: bool = False):
        super().__init__()
        if not float(std) >= 0:
            raise ValueError(f"RandomGaussianNoise: std must not be negative, got {std}")
        self.mean, self.std, self.p, self.same_on_batch, self.keepdim = float(mean), float(std), p, same_on_batch, keepdim
        self._params = None

    def generate_parameters(self, batch_shape):
        return {"batch_prob": _coin(batch_shape[0], self.p, self.same_on_batch), "seed": _field_seed()}

    def forward(self, input: torch.Tensor, params=None) -> torch.Tensor:
        params = self.generate_parameters(input.shape) if params is None else params
        self._params = params
        if input.dtype != torch.float32:
            raise ValueError(f"RandomGaussianNoise: expected a float32 tensor, got {input.dtype}")
        N = input.shape[0]
        win = [n for n in range(N) if bool(params["batch_prob"][n])]
        if not win:
            return input
        rows = input.reshape(N, -1) if len(win) == N else input[win].reshape(len(win), -1)
        noisy = ops.gauss_noise(rows, self.std, int(params["seed"]))
        if self.mean != 0.0:
            noisy = noisy + self.mean
        if len(win) == N:
            return noisy.reshape(input.shape)
        out = input.clone()
        out[win] = noisy.reshape((len(win),) + tuple(input.shape[1:]))
        return out


def _geometric_code(aug, params, n: int):
    """the D4 code of one geometric augmentation per sample, from its drawn parameters"""
    prob = [bool(b) for b in params["batch_prob"]]
    if len(prob) != n:
        raise ValueError(f"{type(aug).__name__}: parameters for {len(prob)} samples, the batch has {n}")
    if isinstance(aug, _RandomFlip):
        if aug.axis not in (-1, -2):
            raise NotImplementedError(f"{type(aug).__name__}: the invertible chain flips the last two axes only")
        return [(4 if aug.axis == -1 else 2) if b else 0 for b in prob]
    times = [int(t) for t in params["times"]]
    return ops.dihedral_codes([0] * n, [0] * n, [t if b else 0 for t, b in zip(times, prob)])


class AugmentationSequential(torch.nn.Module):
    """A chain of this module's augmentations on [N, C, H, W] with per-sample parameters (the part of kornia's
    `AugmentationSequential(..., data_keys=["input"], same_on_batch=False)` the reference uses).  Runs of consecutive geometric
    augmentations (flips, `RandomRotation90`) compose to one code per sample and one `ops.dihedral` launch; `inverse(x,
    params)` undoes the geometric part -- intensity augmentations are not inverted, as in the reference, whose intensity and
    geometric chains are separate containers.  An empty chain returns its input."""
    _NDIM = 4

    def __init__(self, *augmentations: torch.nn.Module, data_keys: Optional[Sequence[str]] = None, same_on_batch: Optional[bool] = None):
        super().__init__()
        if data_keys not in (None, ["input"], ("input",)):
            raise NotImplementedError("AugmentationSequential: data_keys=['input'] only")
        for aug in augmentations:
            if not isinstance(aug, (_RandomFlip, RandomRotation90, RandomGaussianBlur, RandomGaussianNoise)):
                raise NotImplementedError(f"{type(aug).__name__} has no invertible MI355X implementation (flips of the last two "
                                          "axes, RandomRotation90, RandomGaussianBlur and RandomGaussianNoise do)")
            if same_on_batch is not None:
                aug.same_on_batch = same_on_batch
        self.augmentations = torch.nn.ModuleList(augmentations)
        self._params = None

    def _check(self, x):
        if x.dim() != self._NDIM:
            raise RuntimeError(f"Expected {self._NDIM}D tensor, got {tuple(x.shape)}")

    @staticmethod
    def _is_geometric(aug) -> bool:
        return isinstance(aug, (_RandomFlip, RandomRotation90))

    def codes(self, params, n: int):
        """the composed D4 code per sample of the geometric augmentations, for the drawn `params` (one entry per augmentation)"""
        codes = [0] * n
        for aug, p in zip(self.augmentations, params):
            if self._is_geometric(aug):
                codes = [ops.dihedral_compose(c, a) for c, a in zip(codes, _geometric_code(aug, p, n))]
        return codes

    def forward(self, x: torch.Tensor, params=None) -> torch.Tensor:
        self._check(x)
        n, augs = x.shape[0], list(self.augmentations)
        if params is not None and len(params) != len(augs):
            raise ValueError(f"{type(self).__name__}: expected parameters for {len(augs)} augmentations, got {len(params)}")
        used, i = [], 0
        while i < len(augs):
            if not self._is_geometric(augs[i]):
                x = augs[i](x, params=None if params is None else params[i])
                used.append(augs[i]._params)
                i += 1
                continue
            codes = [0] * n
            while i < len(augs) and self._is_geometric(augs[i]):   # one launch for the run
                p = augs[i].generate_parameters(x.shape) if params is None else params[i]
                augs[i]._params = p
                used.append(p)
                codes = [ops.dihedral_compose(c, a) for c, a in zip(codes, _geometric_code(augs[i], p, n))]
                i += 1
            if x.shape[-1] != x.shape[-2] and any(c & 1 for c in codes):
                raise ValueError(f"{type(self).__name__}: a rotation by an odd multiple of 90 degrees was drawn for a non-square patch "
                                 f"({x.shape[-2]} x {x.shape[-1]}); the samples of a batch must share a shape -- use "
                                 "RandomRotation90(times=(0, 0)) or times=(2, 2) for such patches")
            x = ops.dihedral(x, codes)
        self._params = used
        return x

    def inverse(self, x: torch.Tensor, params=None) -> torch.Tensor:
        self._check(x)
        params = self._params if params is None else params
        if params is None:
            raise RuntimeError(f"{type(self).__name__}.inverse: no parameters (call forward first, or pass params=)")
        if not any(self._is_geometric(a) for a in self.augmentations):
            return x
        return ops.dihedral(x, self.codes(params, x.shape[0]), inverse=True)


class AugmentationSequential3D(AugmentationSequential):
    """The same chain on [N, C, D, H, W]: every augmentation acts on the last two axes and depth folds into the planes
    (reference `:89-133`: `(B, C, D, H, W) -> (B, C*D, H, W)` and back).  The kernels take the five axes as they are."""
    _NDIM = 5

    def __init__(self, *augmentations: torch.nn.Module):
        super().__init__(*augmentations)


_CLASSES = {cls.__name__: cls for cls in (RandomHorizontalFlip, RandomVerticalFlip, RandomRotation90, RandomGaussianBlur,
                                           RandomGaussianNoise)}


def _build(ndim, kind, aug_name, aug_dict, p):
    assert ndim == 2 or ndim == 3, f"Number of dimensions must be 2 or 3, got ndim={ndim}"
    assert aug_name is not None or aug_dict is not None, "Either aug_name or aug_dict must be provided."
    if aug_dict is None:
        if aug_name == "weak":
            aug_dict = DEFAULT_WEAK_AUGMENTATIONS[kind]
        elif aug_name == "strong":
            aug_dict = DEFAULT_STRONG_AUGMENTATIONS[kind]
        else:
            raise ValueError(f"Augmentation name needs to be \"weak\" or \"strong\", got aug_name={aug_name}")
    transforms_list = []
    for trafo, kwargs in aug_dict.items():
        assert trafo in _CLASSES, f"{trafo} not found among the invertible augmentations {sorted(_CLASSES)}"
        transforms_list.append(_CLASSES[trafo](p=p, **kwargs))
    if ndim == 2:
        return AugmentationSequential(*transforms_list, data_keys=["input"], same_on_batch=False)
    return AugmentationSequential3D(*transforms_list)


def get_intensity_augmentations(ndim, aug_name: str = None, aug_dict: dict = None, p: float = 0.75) -> Callable:
    return _build(ndim, "intensity", aug_name, aug_dict, p)


def get_geometrical_augmentations(ndim, aug_name: str = None, aug_dict: dict = None, p: float = 0.75) -> Callable:
    return _build(ndim, "geometrical", aug_name, aug_dict, p)


def get_default_augmentations(aug_name: str, ndim: int, p: float = 0.75):
    assert ndim == 2 or ndim == 3, f"Number of dimensions must be 2 or 3, got ndim={ndim}"
    if aug_name not in ("weak", "strong"):
        raise ValueError(f"Augmentation name needs to be \"weak\" or \"strong\", got aug_name={aug_name}")
    return get_intensity_augmentations(ndim, aug_name=aug_name, p=p), get_geometrical_augmentations(ndim, aug_name=aug_name, p=p)


class InvertibleAugmenter(torch.nn.Module):
    """intensity chain, optional clip to [0, clip_max], geometric chain; `reverse_transform` undoes the geometric chain with
    the parameters of the last `transform` (reference `:136-165`)."""

    def __init__(self, intensity_transforms: Callable[[torch.Tensor], torch.Tensor],
                 geometrical_transforms: Callable[[torch.Tensor], torch.Tensor], clip_max=None, **kwargs):
        super().__init__(**kwargs)
        self.intensity_transforms = intensity_transforms
        self.geometrical_transforms = geometrical_transforms
        self.clip_max = clip_max
        self.params = None

    def reset(self):
        self.params = None

    def transform(self, x: torch.Tensor, params=None) -> torch.Tensor:
        """`params` (not in the reference): replay these parameters of the geometric chain instead of drawing"""
        x = self.intensity_transforms(x)
        if self.clip_max is not None:
            x = torch.clamp(x, 0.0, self.clip_max)
        x = self.geometrical_transforms(x) if params is None else self.geometrical_transforms(x, params=params)
        self.params = self.geometrical_transforms._params
        return x

    def reverse_transform(self, x: torch.Tensor) -> torch.Tensor:
        return self.geometrical_transforms.inverse(x, params=self.params)


class _Augmenters:
    _VIEWS = ()

    def reset_all(self):
        for name in self._VIEWS:
            getattr(self, name).reset()


def _default(kind, ndim, clip_max):
    return InvertibleAugmenter(*get_default_augmentations(kind, ndim=ndim), clip_max=clip_max)


class MeanTeacherAugmenters(_Augmenters):
    """`.teacher` and `.student`, both weak by default (reference `:168-181`)"""
    _VIEWS = ("teacher", "student")

    def __init__(self, ndim: int, teacher=None, student=None, clip_max=None):
        self.teacher = teacher or _default("weak", ndim, clip_max)
        self.student = student or _default("weak", ndim, clip_max)


class FixMatchAugmenters(_Augmenters):
    """`.teacher` weak, `.student` strong by default (reference `:184-197`)"""
    _VIEWS = ("teacher", "student")

    def __init__(self, ndim: int, teacher=None, student=None, clip_max=None):
        self.teacher = teacher or _default("weak", ndim, clip_max)
        self.student = student or _default("strong", ndim, clip_max)


class UniMatchv2Augmenters(_Augmenters):
    """`.weak` for the teacher, `.strong1` and `.strong2` for the two student views (reference `:200-216`)"""
    _VIEWS = ("weak", "strong1", "strong2")

    def __init__(self, ndim: int, weak=None, strong1=None, strong2=None, clip_max=None):
        self.weak = weak or _default("weak", ndim, clip_max)
        self.strong1 = strong1 or _default("strong", ndim, clip_max)
        self.strong2 = strong2 or _default("strong", ndim, clip_max)
