"""Full-resolution evaluation: sliding-window, flip and multi-scale inference (csrc/sliding.hip; build-defined, the
reference evaluates the whole image in one forward).

A model trained on crops is evaluated on larger (or arbitrary) images by tiling overlapping crops of the training size,
averaging the overlaps, and optionally averaging over a mirrored copy and a few scales.  The network sees ONE input
shape, [window_batch, 3, ch, cw], whatever the image size is, so the conv engine tunes and allocates once.

window_plan is pure Python.  Everything else runs on the device through three kernels: ssseg_window_gather cuts a batch
of crops, ssseg_window_accumulate upsamples, activates, weights and sums the model's logits of that batch into a
full-resolution accumulator (a gather over accumulator pixels in window-table order: deterministic, and bitwise the
same for every window_batch), ssseg_window_merge divides by the summed weights and resizes to the image.
"""
import torch

from . import native as N
from . import ops

MIRROR, NULL = 1, 2          # window flags (include/ssseg.h)
MAX_WINDOWS = 64             # windows per ssseg_window_accumulate call
ACTIVATIONS = {'none': 0, 'sigmoid': 1, 'softmax': 2}
WEIGHTINGS = {'uniform': 0, 'gaussian': 1}


def _pair(v, name):
    v = (v, v) if isinstance(v, int) else tuple(int(a) for a in v)
    if len(v) != 2 or v[0] < 1 or v[1] < 1:
        raise ValueError(f'{name}: a positive int or (h, w) pair expected, got {v!r}')
    return v


def _axis_origins(size, crop, stride):
    frame = max(size, crop)
    n = -(-(frame - crop) // stride) + 1
    return [min(i * stride, frame - crop) for i in range(n)]


def window_plan(H, W, crop, stride):
    """Origins (y0, x0) of the windows that tile an H x W image with crops of `crop` at `stride` (ints or (h, w) pairs),
    in row-major order.  The working frame is max(H, ch) x max(W, cw) (an image smaller than the crop is zero-padded
    to it); per axis n = ceil((frame - crop) / stride) + 1 windows at min(i * stride, frame - crop): the last window
    is moved back into the frame, never past it."""
    ch, cw = _pair(crop, 'crop')
    sh, sw = _pair(stride, 'stride')
    if H < 1 or W < 1:
        raise ValueError(f'window_plan: empty image {H} x {W}')
    return [(y0, x0) for y0 in _axis_origins(H, ch, sh) for x0 in _axis_origins(W, cw, sw)]


def window_table(rows, device):
    """(device int32 [n,4], host int32 [n,4]) tables of (b, y0, x0, flags) rows."""
    host = torch.tensor(list(rows), dtype=torch.int32).reshape(-1, 4).contiguous()
    return host.to(device), host


def _table(t, name, n=None):
    if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 4 or not t.is_contiguous():
        raise ValueError(f'{name}: a contiguous int32 [n, 4] window table expected')
    if n is not None and t.shape[0] != n:
        raise ValueError(f'{name}: {t.shape[0]} rows for {n} windows')
    return t


def window_gather(image, table, crop, out=None):
    """Crops [n, C, ch, cw] of image [B, C, Hs, Ws] (fp32 or 16-bit) at the rows of the device window table: zeros
    outside the image and for null windows, mirrored where flagged.  `out` (same dtype, any strides) is written in place
    when given."""
    ch, cw = _pair(crop, 'crop')
    if image.dim() != 4:
        raise ValueError('window_gather: [B,C,H,W] image expected')
    ptr = N.dev_ptr(image, 'image')
    _table(table, 'window_gather')
    n = int(table.shape[0])
    B, C, Hs, Ws = image.shape
    if out is None:
        out = torch.empty((n, C, ch, cw), dtype=image.dtype, device=image.device)
    elif tuple(out.shape) != (n, C, ch, cw) or out.dtype != image.dtype:
        raise ValueError(f'window_gather: out must be {(n, C, ch, cw)} {image.dtype}')
    N.call('ssseg_window_gather', ptr, N.strides4(image), B, C, Hs, Ws, N.dev_ptr(table, 'table'), n,
           N.dev_ptr(out, 'out'), N.strides4(out), ch, cw, N.dt_code(image), N.stream())
    return out


def window_accumulate(logits, table, table_host, crop, acc, wsum, activation='softmax', weighting='uniform'):
    """acc [B,C,Ha,Wa] += weight * activation(upsample(logits [n,C,h,w] -> crop)), wsum [B,Ha,Wa] += weight, for the n
    <= 64 windows of the table (device rows, and the same rows on the host for the argument check), in table order."""
    ch, cw = _pair(crop, 'crop')
    if logits.dim() != 4 or acc.dim() != 4 or wsum.dim() != 3:
        raise ValueError('window_accumulate: logits [n,C,h,w], acc [B,C,Ha,Wa], wsum [B,Ha,Wa] expected')
    ptr = N.dev_ptr(logits, 'logits')
    n, C, h, w = logits.shape
    B, Ca, Ha, Wa = acc.shape
    if logits.dtype != torch.float32 or acc.dtype != torch.float32 or wsum.dtype != torch.float32:
        raise ValueError('window_accumulate: fp32 logits, acc and wsum expected')
    if Ca != C or tuple(wsum.shape) != (B, Ha, Wa) or not acc.is_contiguous() or not wsum.is_contiguous():
        raise ValueError('window_accumulate: acc [B,C,Ha,Wa] and wsum [B,Ha,Wa] must be contiguous and match the logits')
    _table(table, 'window_accumulate', n)
    _table(table_host, 'window_accumulate (host)', n)
    if table_host.is_cuda:
        raise ValueError('window_accumulate: table_host must be a CPU tensor')
    N.call('ssseg_window_accumulate', ptr, N.strides4(logits), n, C, h, w, N.dev_ptr(table, 'table'),
           table_host.data_ptr(), ch, cw, ACTIVATIONS[activation], WEIGHTINGS[weighting], N.dev_ptr(acc, 'acc'),
           N.dev_ptr(wsum, 'wsum'), B, Ha, Wa, N.stream())


def window_merge(acc, wsum, interior, out, scale_weight=1.0, first=True):
    """out [B,C,H,W] = (first) or += scale_weight * bilinear(acc / wsum) sampled from the `interior` (Hs, Ws) of the
    accumulator; exactly acc / wsum * scale_weight where the interior has the output's size."""
    Hs, Ws = interior
    B, C, Ha, Wa = acc.shape
    if tuple(out.shape[:2]) != (B, C) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError('window_merge: out must be contiguous fp32 [B,C,H,W]')
    N.call('ssseg_window_merge', N.dev_ptr(acc, 'acc'), N.dev_ptr(wsum, 'wsum'), B, C, Ha, Wa, int(Hs), int(Ws),
           N.dev_ptr(out, 'out'), int(out.shape[2]), int(out.shape[3]), float(scale_weight), int(bool(first)),
           N.stream())
    return out


def argmax_labels(x):
    """[B,H,W] int64 argmax over the channels of fp32 [B,C,H,W] (first maximum)."""
    x = x if x.is_contiguous() else x.contiguous()
    B, C, H, W = x.shape
    out = torch.empty((B, H, W), dtype=torch.int64, device=x.device)
    N.call('ssseg_window_argmax', N.dev_ptr(x, 'x'), B, C, H * W, N.dev_ptr(out), N.stream())
    return out


class SlidingWindowInference:
    """model: the repository's usual `features, [logits...]` model (the last logit map is used, at whatever resolution
    the model emits it).  __call__(image [B,3,H,W]) -> fp32 [B,C,H,W]: the mean over windows, mirrored copies and
    scales of the activated output ('softmax', 'sigmoid'), or of the logits ('none').

    Per scale s the image is resized to (int(H s + 0.5), int(W s + 0.5)) (s = 1: the image itself), tiled by
    window_plan, and the window list -- every plan window of every image, then the same list mirrored when flip is set,
    then null windows up to a multiple of window_batch -- is fed window_batch crops at a time.  The device window
    tables are cached per (B, H, W, scale): a second call on the same shape copies nothing from the host."""

    def __init__(self, model, crop_size, stride=None, scales=(1.0,), flip=False, activation='softmax',
                 weighting='uniform', window_batch=8):
        self.model = model
        self.crop = _pair(crop_size, 'crop_size')
        self.stride = tuple(-(-2 * c // 3) for c in self.crop) if stride is None else _pair(stride, 'stride')
        self.scales = tuple(float(s) for s in scales)
        if not self.scales or min(self.scales) <= 0:
            raise ValueError(f'SlidingWindowInference: positive scales expected, got {scales!r}')
        if activation not in ACTIVATIONS:
            raise ValueError(f'SlidingWindowInference: activation must be one of {sorted(ACTIVATIONS)}')
        if weighting not in WEIGHTINGS:
            raise ValueError(f'SlidingWindowInference: weighting must be one of {sorted(WEIGHTINGS)}')
        if int(window_batch) < 1:
            raise ValueError('SlidingWindowInference: window_batch must be at least 1')
        self.flip, self.activation, self.weighting = bool(flip), activation, weighting
        self.window_batch = int(window_batch)
        self._tables = {}

    def windows(self, B, Hs, Ws):
        """the padded window list of one scale: rows (b, y0, x0, flags)"""
        plan = window_plan(Hs, Ws, self.crop, self.stride)
        rows = [(b, y0, x0, 0) for b in range(B) for y0, x0 in plan]
        if self.flip:
            rows += [(b, y0, x0, MIRROR) for b, y0, x0, _ in rows]
        rows += [(0, 0, 0, NULL)] * (-len(rows) % self.window_batch)
        return rows

    def _scale_tables(self, B, H, W, s, device):
        key = (B, H, W, s, str(device))
        hit = self._tables.get(key)
        if hit is None:
            Hs, Ws = (H, W) if s == 1.0 else (int(H * s + 0.5), int(W * s + 0.5))
            if Hs < 1 or Ws < 1:
                raise ValueError(f'SlidingWindowInference: scale {s} of a {H} x {W} image is empty')
            dev, host = window_table(self.windows(B, Hs, Ws), device)
            hit = (Hs, Ws, dev, host)
            self._tables[key] = hit
        return hit

    def __call__(self, image):
        if image.dim() != 4:
            raise ValueError('SlidingWindowInference: [B,3,H,W] image batch expected')
        N.dev_ptr(image, 'image')
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                return self._run(image)
        finally:
            self.model.train(was_training)

    def _run(self, image):
        B, Cimg, H, W = image.shape
        ch, cw = self.crop
        wb = self.window_batch
        crops = torch.empty((wb, Cimg, ch, cw), dtype=image.dtype, device=image.device)
        out = None
        for si, s in enumerate(self.scales):
            Hs, Ws, table, table_host = self._scale_tables(B, H, W, s, image.device)
            img = image if (Hs, Ws) == (H, W) else ops.interpolate_bilinear(image, (Hs, Ws), align_corners=False)
            Ha, Wa = max(Hs, ch), max(Ws, cw)
            acc = wsum = None
            for k in range(0, int(table.shape[0]), wb):
                window_gather(img, table[k:k + wb], self.crop, out=crops)
                _, logit_maps = self.model(crops)
                logits = logit_maps[-1]
                if logits.dim() != 4 or logits.shape[0] != wb:
                    raise RuntimeError(f'SlidingWindowInference: the model returned {tuple(logits.shape)} for '
                                       f'{wb} crops')
                if logits.dtype != torch.float32:
                    logits = logits.float()
                if acc is None:
                    C = int(logits.shape[1])
                    acc = torch.zeros((B, C, Ha, Wa), dtype=torch.float32, device=image.device)
                    wsum = torch.zeros((B, Ha, Wa), dtype=torch.float32, device=image.device)
                    if out is None:
                        out = torch.empty((B, C, H, W), dtype=torch.float32, device=image.device)
                for q in range(0, wb, MAX_WINDOWS):
                    window_accumulate(logits[q:q + MAX_WINDOWS], table[k + q:k + min(q + MAX_WINDOWS, wb)],
                                      table_host[k + q:k + min(q + MAX_WINDOWS, wb)], self.crop, acc, wsum,
                                      self.activation, self.weighting)
            window_merge(acc, wsum, (Hs, Ws), out, 1.0 / len(self.scales), first=si == 0)
        return out

    def predict(self, image):
        """[B,H,W] int64 labels: the argmax (first maximum) of the fused map."""
        return argmax_labels(self(image))
