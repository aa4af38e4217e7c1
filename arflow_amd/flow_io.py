""".flo reader / writer and the end-point-error definition of the reference
(utils/flow_utils.py:23-32 load, :35-65 write_flow, :145-148 EPE), numpy only (the reference needs cv2); binary PPM / PGM
writers for the rendered flow and entropy pictures (arflow_amd.render), numpy only as well."""
import os

import numpy as np

FLO_MAGIC = np.float32(202021.25)


def write_flow(filename, uv):
    """uv: [H, W, 2] float array (u, v) -> Middlebury .flo (magic, width, height, interleaved u,v rows)."""
    uv = np.asarray(uv, dtype=np.float32)
    assert uv.ndim == 3 and uv.shape[2] == 2
    h, w = uv.shape[:2]
    with open(filename, 'wb') as f:
        np.array([FLO_MAGIC], np.float32).tofile(f)
        np.array([w, h], np.int32).tofile(f)
        uv.tofile(f)


def read_flow(filename):
    with open(filename, 'rb') as f:
        magic = np.fromfile(f, np.float32, count=1)
        if magic.size != 1 or magic[0] != FLO_MAGIC:
            raise ValueError('Magic number incorrect. Invalid .flo file')
        w, h = np.fromfile(f, np.int32, count=2)
        data = np.fromfile(f, np.float32, count=2 * int(w) * int(h))
    return data.reshape(int(h), int(w), 2)


def epe(pred, gt):
    """Mean end-point error between two [H, W, 2] flows of the same size."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    return float(np.sqrt(((pred[..., :2] - gt[..., :2]) ** 2).sum(-1)).mean())


def _write_pnm(path, magic, a, shape_ok, what):
    a = np.asarray(a)
    if a.dtype != np.uint8 or not shape_ok(a):
        raise ValueError('%s (got %s %s)' % (what, a.dtype, a.shape))
    with open(path, 'wb') as f:
        f.write(b'%s\n%d %d\n255\n' % (magic, a.shape[1], a.shape[0]))
        np.ascontiguousarray(a).tofile(f)


def write_ppm(path, rgb):
    """rgb: uint8 [H, W, 3] -> binary PPM (P6)."""
    _write_pnm(path, b'P6', rgb, lambda a: a.ndim == 3 and a.shape[2] == 3, 'write_ppm takes a uint8 [H,W,3] array')


def write_pgm(path, gray):
    """gray: uint8 [H, W] -> binary PGM (P5)."""
    _write_pnm(path, b'P5', gray, lambda a: a.ndim == 2, 'write_pgm takes a uint8 [H,W] array')


def write_image(path, array):
    """uint8 [H,W,3] or [H,W] by extension: .ppm / .pgm through the writers above, .png through PIL (the package
    arflow_amd.inference.load_image needs already).  Anything else is refused."""
    ext = os.path.splitext(path)[1].lower()
    array = np.asarray(array)
    if ext in ('.ppm', '.pgm'):
        if (ext == '.ppm') != (array.ndim == 3):
            raise ValueError('%s holds %s images (got shape %s)' % (ext, 'colour' if ext == '.ppm' else 'grey', array.shape))
        return write_ppm(path, array) if ext == '.ppm' else write_pgm(path, array)
    if ext == '.png':
        from PIL import Image
        if array.dtype != np.uint8 or not (array.ndim == 2 or (array.ndim == 3 and array.shape[2] == 3)):
            raise ValueError('write_image takes a uint8 [H,W,3] or [H,W] array (got %s %s)' % (array.dtype, array.shape))
        return Image.fromarray(array).save(path)
    raise ValueError('write_image writes .ppm, .pgm and .png (got %r)' % (path,))
