"""Defect augmentation for EM volumes (reference `transform/defect.py:41-245`): per z-slice one uniform draw picks one of
leave / drop / low contrast / deform / paste an artifact.

numpy input runs the reference's algorithm with the reference's `np.random` draws in the reference's order, on scipy alone:
`scipy.ndimage.gaussian_filter(sigma=3, mode="nearest", truncate=4.0)` stands for `skimage.filters.gaussian`, `line()` below
(an integer Bresenham) for `skimage.draw.line`, and the per-row (per-column) interval of the line for the two labelled
components of `bioimage_cpp.segmentation.label`.  Neither skimage nor bioimage_cpp is a dependency of this package or of
its fixtures, so parity with those three functions is UNPINNED (as for kornia in `invertible_augmentations.py`); everything else
of the numpy branch is pinned draw for draw by tests/golden/g20_defect.npz, recorded from the reference's class with
these stand-ins.

A CUDA tensor `[Z, H, W]` runs on the device (csrc/defect.hip).  `sample_plan` draws the per-slice scalars
on the host from numpy's global state in the reference's order -- per slice `r`, then the coin of mode "all", then the
compress draws `rand, randint, randint`, then the artifact index -- and one `_field_seed()` at the end if any slice
deforms.  The noise FIELDS come from the package's counter-based stream (`_philox.py`), not from numpy's: field f (0: the
displacement along columns, 1: along rows) of slice s is stream row 2 s + f, element r * W + c, so a slice's noise does
not depend on what happens to the other slices.  `apply_plan` replays a plan; `__call__` is one after the other.
`per_sample=True` (not in the reference) takes `[N, Z, H, W]` or `[N, 1, Z, H, W]` and treats all N * Z slices in the same
launches, s counting through the batch: usable as the `prepass` of `DevicePrefetcher`.

Not built: `get_artifact_source` (it needs the reference's lazy file datasets and `MinForegroundSampler`, which this
package does not have).  `artifact_source` is any sequence-like dataset yielding `(artifact, alpha_mask)`.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .raw import _field_seed

KEEP, DROP, LOW_CONTRAST, DEFORM, PASTE = "keep", "drop", "low_contrast", "deform", "paste"
SIGMA, TRUNCATE = 3.0, 4.0     # of the smoothed flow (hard-coded in the reference)
BAND = 10                      # dilation steps around a compress line
SPLINE_POLE = np.sqrt(3.0) - 2.0
SPLINE_RADIUS = 16             # taps a side of the prefilter's impulse response: |pole|^17 < 2e-10


# ---------------------------------------------------------------------------
# host geometry: line, interval table, sides, band
# ---------------------------------------------------------------------------
def line(r0: int, c0: int, r1: int, c1: int) -> Tuple[np.ndarray, np.ndarray]:
    """The pixels of the Bresenham line from (r0, c0) to (r1, c1), both included, in that order.  The line is always
    generated from the lexicographically smaller endpoint, so swapping the endpoints gives the same pixels reversed."""
    r0, c0, r1, c1 = int(r0), int(c0), int(r1), int(c1)
    swap = (r0, c0) > (r1, c1)
    if swap:
        r0, c0, r1, c1 = r1, c1, r0, c0
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sr, sc = (1 if r1 >= r0 else -1), (1 if c1 >= c0 else -1)
    n = max(dr, dc)
    rr, cc = np.empty(n + 1, dtype=np.int64), np.empty(n + 1, dtype=np.int64)
    r, c, err = r0, c0, 2 * min(dr, dc) - n
    for i in range(n + 1):
        rr[i], cc[i] = r, c
        if err > 0:
            if dr > dc:
                c += sc
            else:
                r += sr
            err -= 2 * n
        if dr > dc:
            r += sr
        else:
            c += sc
        err += 2 * min(dr, dc)
    return (rr[::-1].copy(), cc[::-1].copy()) if swap else (rr, cc)


def line_intervals(rr, cc, shape, by_rows: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) per row (by_rows: the line runs from the first row to the last) or per column: the line covers lo..hi there"""
    a, b = (rr, cc) if by_rows else (cc, rr)
    n = shape[0] if by_rows else shape[1]
    lo, hi = np.full(n, np.iinfo(np.int64).max), np.full(n, -1)
    np.minimum.at(lo, a, b)
    np.maximum.at(hi, a, b)
    if (hi < 0).any():
        raise ValueError("the line does not cross the whole slice")
    return lo, hi


def sides(lo, hi, shape, by_rows: bool) -> np.ndarray:
    """int8 [H, W]: +1 on the side whose flow is +strength * normal, -1 on the other, 0 on the line.  by_rows: the pixels
    right of the line are the positive side (the reference's component of the last pixel); else those above it (the
    component of the first pixel)."""
    r, c = np.mgrid[:shape[0], :shape[1]]
    if by_rows:
        return (c > hi[:, None]).astype(np.int8) - (c < lo[:, None]).astype(np.int8)
    return (r < lo[None, :]).astype(np.int8) - (r > hi[None, :]).astype(np.int8)


def band(lo, hi, shape, by_rows: bool, steps: int = BAND) -> np.ndarray:
    """bool [H, W]: L1 distance to a pixel of the line <= steps (`binary_dilation(line_mask, iterations=steps)`)"""
    n, m = (shape[0], shape[1]) if by_rows else (shape[1], shape[0])
    b = np.arange(m)[None, :]
    out = np.zeros((n, m), dtype=bool)
    for da in range(-steps, steps + 1):
        a0, a1 = max(0, -da), min(n, n - da)          # rows a with a + da inside
        if a0 >= a1:
            continue
        l, h = lo[a0 + da:a1 + da, None], hi[a0 + da:a1 + da, None]
        dist = np.where(b < l, l - b, np.where(b > h, b - h, 0))
        out[a0:a1] |= dist <= steps - abs(da)
    return out if by_rows else out.T


def gaussian_weights(sigma: float = SIGMA, truncate: float = TRUNCATE) -> np.ndarray:
    """scipy's weights of `gaussian_filter(sigma, truncate)`: radius int(truncate * sigma + 0.5), float64"""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def spline_fir_weights(radius: int = SPLINE_RADIUS) -> np.ndarray:
    """The two-sided impulse response sqrt(3) * pole^|k| of the cubic B-spline prefilter (pole sqrt(3) - 2, gain 6), cut
    after `radius` taps a side; float64.  On the whole-sample mirror extension it gives `spline_filter(order=3,
    mode="mirror")` up to |pole|^(radius + 1)."""
    k = np.abs(np.arange(-radius, radius + 1))
    return np.sqrt(3.0) * SPLINE_POLE ** k


def stream_row(slice_index: int, field: int) -> int:
    """the stream row of noise field `field` (0: along columns, 1: along rows) of slice `slice_index` of the batch"""
    return 2 * int(slice_index) + int(field)


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------
class DefectPlan:
    """What `sample_plan` drew: per slice an action and its scalars, and the seed of the noise fields.
    actions[s]: KEEP / DROP / LOW_CONTRAST / DEFORM / PASTE; deform[s]: None, ("undirected",) or ("compress", fixed_x,
    (x0, y0, x1, y1)) with the reference's endpoint names (x: row, y: column); artifact[s]: index into the source or -1."""

    def __init__(self, shape, actions, deform, artifact, seed):
        self.shape, self.actions, self.deform, self.artifact, self.seed = tuple(shape), list(actions), list(deform), list(artifact), seed

    @property
    def n_slices(self) -> int:
        return len(self.actions)

    @property
    def deformed(self) -> List[int]:
        return [s for s, a in enumerate(self.actions) if a == DEFORM]


def compress_flow(endpoints, strength: float) -> Tuple[np.float32, np.float32]:
    """(flow along columns, flow along rows) of the positive side of a compress line, rounded as the reference rounds them"""
    x0, y0, x1, y1 = endpoints
    vec = np.array([x1 - x0, y1 - y0], dtype="float32")
    vec /= np.linalg.norm(vec)
    normal = np.zeros_like(vec)
    normal[0], normal[1] = -vec[1], vec[0]
    return np.float32(strength * normal[1]), np.float32(strength * normal[0])


class EMDefectAugmentation:
    """Augment raw data with transformations similar to defects common in EM data (reference `:41-245`; same arguments,
    cumulative probabilities and assertions).

    Args:
        p_drop_slice: Probability for a missing slice.
        p_low_contrast: Probability for a low contrast slice.
        p_deform_slice: Probability for a deformed slice.
        p_paste_artifact: Probability for inserting an artifact from data source.
        contrast_scale: Scale of low contrast transformation.
        deformation_mode: "undirected", "compress" or "all" (or a list of the first two).
        deformation_strength: Deformation strength in pixel.
        artifact_source: Data source for additional artifacts, yielding (artifact, alpha_mask).
        mean_val: Mean value for artifact normalization; the fill value of a compressed slice.
        std_val: Std value for artifact normalization (kept, unused, as in the reference).
        per_sample: Device only, not in the reference: the first axis is a batch axis.
    """

    def __init__(self, p_drop_slice: float, p_low_contrast: float, p_deform_slice: float, p_paste_artifact: float = 0.0,
                 contrast_scale: float = 0.1, deformation_mode="undirected", deformation_strength: float = 10.0,
                 artifact_source=None, mean_val: Optional[float] = None, std_val: Optional[float] = None, per_sample: bool = False):
        if p_paste_artifact > 0.0:
            assert artifact_source is not None
        self.artifact_source = artifact_source
        self.p_drop_slice = p_drop_slice
        self.p_low_contrast = self.p_drop_slice + p_low_contrast
        self.p_deform_slice = self.p_low_contrast + p_deform_slice
        self.p_paste_artifact = self.p_deform_slice + p_paste_artifact
        assert self.p_paste_artifact < 1.0
        self.contrast_scale = contrast_scale
        self.mean_val = mean_val
        self.std_val = std_val
        if isinstance(deformation_mode, str):
            assert deformation_mode in ("all", "undirected", "compress")
            self.deformation_mode = deformation_mode
        elif isinstance(deformation_mode, (list, tuple)):
            assert len(deformation_mode) == 2
            assert "undirected" in deformation_mode
            assert "compress" in deformation_mode
            self.deformation_mode = "all"
        self.deformation_strength = deformation_strength
        self.per_sample = per_sample

    # ---- shared draws ----
    def _action(self, r: float) -> str:
        if r < self.p_drop_slice:
            return DROP
        if r < self.p_low_contrast:
            return LOW_CONTRAST
        if r < self.p_deform_slice:
            return DEFORM
        if r < self.p_paste_artifact:
            return PASTE
        return KEEP

    def _draw_mode(self) -> str:
        if self.deformation_mode in ("undirected", "compress"):
            return self.deformation_mode
        return "undirected" if np.random.rand() < .5 else "compress"

    @staticmethod
    def _draw_line(shape):
        fixed_x = bool(np.random.rand() < .5)
        if fixed_x:
            x0, y0 = 0, np.random.randint(1, shape[1] - 2)
            x1, y1 = shape[0] - 1, np.random.randint(1, shape[1] - 2)
        else:
            x0, y0 = np.random.randint(1, shape[0] - 2), 0
            x1, y1 = np.random.randint(1, shape[0] - 2), shape[1] - 1
        return fixed_x, (int(x0), int(y0), int(x1), int(y1))

    @staticmethod
    def _check_shape(shape, mode):
        if min(shape) < 4:
            raise ValueError(f"EMDefectAugmentation: slices of at least 4 x 4 pixels, got {tuple(shape)}")
        if mode == "undirected" and shape[0] != shape[1]:
            raise ValueError(f"EMDefectAugmentation: undirected deformation needs square slices, got {tuple(shape)} "
                             "(the reference's grid is transposed and fails to broadcast)")

    # ---- numpy branch: the reference's arithmetic ----
    def _compress_numpy(self, raw):
        from scipy.ndimage import map_coordinates
        shape = raw.shape
        fixed_x, ends = self._draw_line(shape)
        lo, hi = line_intervals(*line(*ends), shape, fixed_x)
        side = sides(lo, hi, shape, fixed_x)
        pos_x, pos_y = compress_flow(ends, self.deformation_strength)
        cols, rows = np.meshgrid(np.arange(shape[1]), np.arange(shape[0]))
        flow_x, flow_y = np.zeros_like(raw), np.zeros_like(raw)
        flow_x[side > 0], flow_x[side < 0] = pos_x, -pos_x
        flow_y[side > 0], flow_y[side < 0] = pos_y, -pos_y
        flow_x += np.random.uniform(-1, 1, shape) * (self.deformation_strength / 8.)
        flow_y += np.random.uniform(-1, 1, shape) * (self.deformation_strength / 8.)
        at = ((rows + flow_y).reshape(-1, 1), (cols + flow_x).reshape(-1, 1))
        cval = 0.0 if self.mean_val is None else self.mean_val
        out = map_coordinates(raw, at, mode="constant", order=3, cval=cval).reshape(shape)
        out[band(lo, hi, shape, fixed_x)] = 0.
        return out

    def _undirected_numpy(self, raw):
        from scipy.ndimage import gaussian_filter, map_coordinates
        shape = raw.shape
        cols, rows = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]))
        flow_x = np.random.uniform(-1, 1, shape) * self.deformation_strength
        flow_y = np.random.uniform(-1, 1, shape) * self.deformation_strength
        flow_x = gaussian_filter(flow_x, sigma=SIGMA, mode="nearest", truncate=TRUNCATE)
        flow_y = gaussian_filter(flow_y, sigma=SIGMA, mode="nearest", truncate=TRUNCATE)
        at = ((rows + flow_y).reshape(-1, 1), (cols + flow_x).reshape(-1, 1))
        return map_coordinates(raw, at, mode="constant").reshape(shape)

    def _paste_numpy(self, raw):
        index = np.random.randint(len(self.artifact_source))
        artifact, alpha = self._artifact(index, raw.shape)
        return raw * (1. - alpha) + artifact * alpha

    def _artifact(self, index, shape):
        artifact, alpha = self.artifact_source[index]
        artifact, alpha = np.asarray(artifact.cpu() if torch.is_tensor(artifact) else artifact).squeeze(), \
            np.asarray(alpha.cpu() if torch.is_tensor(alpha) else alpha).squeeze()
        assert artifact.shape == tuple(shape), f"{artifact.shape}, {tuple(shape)}"
        assert alpha.shape == tuple(shape)
        assert alpha.min() >= 0., f"{alpha.min()}"
        assert alpha.max() <= 1., f"{alpha.max()}"
        return artifact, alpha

    def _numpy(self, raw):
        raw = np.asarray(raw).astype("float32")
        for z in range(raw.shape[0]):
            action = self._action(np.random.rand())
            if action == DROP:
                raw[z] = 0
            elif action == LOW_CONTRAST:
                sl = raw[z]
                mean = sl.mean()
                sl -= mean
                sl *= self.contrast_scale
                sl += mean
            elif action == DEFORM:
                mode = self._draw_mode()
                self._check_shape(raw[z].shape, mode)
                raw[z] = self._compress_numpy(raw[z]) if mode == "compress" else self._undirected_numpy(raw[z])
            elif action == PASTE:
                raw[z] = self._paste_numpy(raw[z])
        return raw

    # ---- device branch ----
    def sample_plan(self, n_slices: int, shape: Sequence[int]) -> DefectPlan:
        """Draws the plan of `n_slices` slices of `shape` (H, W) from numpy's global state (order: module docstring)."""
        shape = (int(shape[0]), int(shape[1]))
        self._check_shape(shape, None)
        actions, deform, artifact = [], [], []
        for _ in range(int(n_slices)):
            action = self._action(np.random.rand())
            d, a = None, -1
            if action == DEFORM:
                mode = self._draw_mode()
                self._check_shape(shape, mode)
                d = ("compress", *self._draw_line(shape)) if mode == "compress" else ("undirected",)
            elif action == PASTE:
                a = int(np.random.randint(len(self.artifact_source)))
            actions.append(action)
            deform.append(d)
            artifact.append(a)
        seed = _field_seed() if DEFORM in actions else None
        return DefectPlan(shape, actions, deform, artifact, seed)

    def plan_tables(self, plan: DefectPlan):
        """(plan int32 [S, 4], rec int32 [D, 8], tables int32, artifact indices in plane order): the device tables of a
        plan (include/tem_hip.h), as numpy arrays"""
        from .. import ops
        H, W = plan.shape
        code = {KEEP: ops.DEFECT_KEEP, DROP: ops.DEFECT_DROP, LOW_CONTRAST: ops.DEFECT_LOW, PASTE: ops.DEFECT_PASTE,
                DEFORM: ops.DEFECT_DEFORM}
        ptab = np.zeros((plan.n_slices, 4), dtype=np.int32)
        ptab[:, 0] = [code[a] for a in plan.actions]
        ptab[:, 2] = np.float32(self.contrast_scale).view(np.int32)
        pasted = [s for s, a in enumerate(plan.actions) if a == PASTE]
        ptab[pasted, 1] = np.arange(len(pasted))
        rec = np.zeros((len(plan.deformed), 8), dtype=np.int32)
        recf = rec.view(np.float32)
        tables = []
        for d, s in enumerate(plan.deformed):
            rec[d, 0], rec[d, 3] = s, stream_row(s, 0)
            recf[d, 6] = 0.0
            if plan.deform[s][0] == "compress":
                _, fixed_x, ends = plan.deform[s]
                lo, hi = line_intervals(*line(*ends), plan.shape, fixed_x)
                rec[d, 1], rec[d, 2] = (1 if fixed_x else 2), sum(len(t) for t in tables)
                recf[d, 4], recf[d, 5] = compress_flow(ends, self.deformation_strength)
                recf[d, 6] = 0.0 if self.mean_val is None else self.mean_val
                tables.append((lo | (hi << 16)).astype(np.int32))
        tables = np.concatenate(tables) if tables else np.zeros(0, dtype=np.int32)
        return ptab, rec, tables, [plan.artifact[s] for s in pasted]

    def apply_plan(self, raw: torch.Tensor, plan: DefectPlan, seed: Optional[int] = None) -> torch.Tensor:
        """Applies `plan` to the CUDA tensor `raw` ([Z, H, W]; per_sample: [N, Z, H, W] or [N, 1, Z, H, W]); the noise fields
        come from `seed` (default: the plan's).  Returns a new float32 tensor of raw's shape; `raw` is not modified."""
        from .. import ops
        if not (torch.is_tensor(raw) and raw.is_cuda):
            raise RuntimeError("EMDefectAugmentation.apply_plan runs on MI355X only; numpy input goes through __call__")
        x = self._as_slices(raw)
        if (x.shape[0], tuple(x.shape[1:])) != (plan.n_slices, plan.shape):
            raise ValueError(f"the plan was drawn for {plan.n_slices} slices of {plan.shape}, got {tuple(x.shape)}")
        H, W = plan.shape
        ptab, rec, tables, chosen = self.plan_tables(plan)
        tab = ops.DefectTables(ptab, rec, tables, plan.n_slices, H, W, len(chosen), x.device)
        art = alpha = None
        if chosen:
            pairs = [self._artifact(i, plan.shape) for i in chosen]
            art = ops._to_device(np.stack([p[0] for p in pairs]).astype(np.float32), x.device)
            alpha = ops._to_device(np.stack([p[1] for p in pairs]).astype(np.float32), x.device)
        y = ops.defect_apply(x, tab, ops.defect_mean(x, tab), art, alpha)
        if tab.D:
            seed = plan.seed if seed is None else seed
            if seed is None:
                raise ValueError("a plan with deformed slices needs a seed")
            ws = ops._workspace(3 * tab.D * H * W * 4, x.device)[:3 * tab.D * H * W * 4].view(torch.float32)
            coef, flow = ws[:tab.D * H * W].view(tab.D, H, W), ws[tab.D * H * W:].view(tab.D, 2, H, W)
            strength = float(self.deformation_strength)
            ops.defect_prefilter(x, tab, spline_fir_weights(), out=coef)
            if (rec[:, 1] == 0).any():
                ops.defect_flow(tab, seed, strength, gaussian_weights(), out=flow)
            ops.defect_warp(coef, flow, y, tab, seed, strength / 8.)
        return y.reshape(raw.shape)

    def _as_slices(self, raw: torch.Tensor) -> torch.Tensor:
        ok = (4, 5) if self.per_sample else (3,)
        if raw.dim() not in ok or (raw.dim() == 5 and raw.shape[1] != 1):
            raise ValueError(f"EMDefectAugmentation: expected {'[N, Z, H, W] or [N, 1, Z, H, W]' if self.per_sample else '[Z, H, W]'}, "
                             f"got {tuple(raw.shape)}")
        return raw.float().contiguous().reshape(-1, raw.shape[-2], raw.shape[-1])

    def __call__(self, raw):
        """Apply defect augmentations to input data: a numpy array [Z, H, W] (the reference's path) or a CUDA tensor."""
        if torch.is_tensor(raw) and raw.is_cuda:
            x = self._as_slices(raw)
            return self.apply_plan(raw, self.sample_plan(x.shape[0], x.shape[1:]))
        if torch.is_tensor(raw):
            raise RuntimeError("EMDefectAugmentation: a CPU tensor has no path here (numpy arrays run the reference's algorithm, "
                               "CUDA tensors the device kernels)")
        if self.per_sample:
            raise ValueError("EMDefectAugmentation: per_sample is a device option")
        return self._numpy(raw)
