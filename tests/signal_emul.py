"""numpy restatement of rcb_signal_patch (include/rcb.h, N4), written from its definition -- not from the kernel:

    y row n = patch n % prod(patch_nums), row-major over patch_nums, of signal n // prod(patch_nums); its pixels the row-major
              positions inside the patch; uint8 sources as q / 255 in fp32 (one division), fp32 sources unchanged

The patches are cut with one slice each, in nested loops over the patch index, the way the reference's loaders do
(data/image.py:30-46); no index arithmetic is shared with the kernel, nor with recon_emul.stitch (reshape / transpose), whose
inverse this is."""
import itertools

import numpy as np

F32 = np.float32


def unit8(q):
    """uint8 -> fp32 in [0, 1]: one fp32 division by 255"""
    v = F32(q) / F32(255) if np.isscalar(q) else np.asarray(q).astype(F32) / F32(255)
    assert v.dtype == F32
    return v


def patch(view, patch_nums, patch_size):
    """view [n, *G, C] with G_i = patch_nums[i] * patch_size[i] (any numpy array, any strides) -> [n * prod(patch_nums),
    prod(patch_size), C], same dtype, values untouched"""
    view = np.asarray(view)
    pn, ps = list(patch_nums), list(patch_size)
    nd = len(pn)
    assert view.ndim == nd + 2 and tuple(view.shape[1:-1]) == tuple(a * b for a, b in zip(pn, ps))
    C = view.shape[-1]
    rows = []
    for d in range(view.shape[0]):
        for b in itertools.product(*[range(k) for k in pn]):             # row-major over patch_nums
            cut = view[d][tuple(slice(b[i] * ps[i], (b[i] + 1) * ps[i]) for i in range(nd))]
            rows.append(cut.reshape(-1, C))                              # row-major inside the patch
    if not rows:
        return np.zeros((0, int(np.prod(ps)), C), dtype=view.dtype)
    return np.stack(rows)


def targets(view, patch_nums, patch_size):
    """what rcb_signal_patch writes: fp32 [N, P, C]"""
    out = patch(view, patch_nums, patch_size)
    return unit8(out) if out.dtype == np.uint8 else out.astype(F32, copy=False)


def bits(a):
    """fp32 array -> its int32 bit patterns (NaN payloads and the sign of zero compare)"""
    a = np.ascontiguousarray(a)
    assert a.dtype == F32
    return a.view(np.int32)
