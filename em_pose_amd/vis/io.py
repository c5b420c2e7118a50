"""Images of the renderer to disk: PNG through PIL where it is installed (imported lazily), else binary PPM with the
standard library alone."""
import os

import numpy as np


def _to_numpy(rgb):
    if hasattr(rgb, 'detach'):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.shape[-1] != 3:
        raise ValueError('images must be uint8 (..., H, W, 3)')
    return rgb


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def save_image(path_without_suffix, image):
    """One (H, W, 3) uint8 image -> `<path>.png`, or `<path>.ppm` without PIL; returns the path written."""
    image = _to_numpy(image)
    if image.ndim != 3:
        raise ValueError('one image is (H, W, 3)')
    Image = _pil()
    if Image is not None:
        path = path_without_suffix + '.png'
        Image.fromarray(image).save(path)
        return path
    path = path_without_suffix + '.ppm'
    with open(path, 'wb') as f:
        f.write(b'P6\n%d %d\n255\n' % (image.shape[1], image.shape[0]))
        f.write(image.tobytes())
    return path


def save_frames(directory, rgb, prefix='frame_', start=0, step=1):
    """(T, H, W, 3) uint8 -> `<directory>/<prefix>NNNNNN.png` (or .ppm), numbered start, start + step, ...; returns
    the paths."""
    rgb = _to_numpy(rgb)
    if rgb.ndim != 4:
        raise ValueError('frames are (T, H, W, 3)')
    os.makedirs(directory, exist_ok=True)
    return [save_image(os.path.join(directory, '%s%06d' % (prefix, start + k * step)), rgb[k])
            for k in range(rgb.shape[0])]


def side_by_side(*rgbs):
    """Images or stacks of images of equal height, next to each other (concatenated along the width)."""
    if hasattr(rgbs[0], 'detach'):
        import torch
        return torch.cat(list(rgbs), dim=-2)
    return np.concatenate([_to_numpy(r) for r in rgbs], axis=-2)


def contact_sheet(rgb_list, columns):
    """Equal-sized (H, W, 3) images -> one (rows * H, columns * W, 3) uint8 array, row-major; cells left over are
    white."""
    images = [_to_numpy(im) for im in rgb_list]
    if not images or columns < 1:
        raise ValueError('contact_sheet needs at least one image and one column')
    h, w = images[0].shape[:2]
    if any(im.shape != (h, w, 3) for im in images):
        raise ValueError('contact_sheet needs images of one size')
    rows = (len(images) + columns - 1) // columns
    sheet = np.full((rows * h, columns * w, 3), 255, dtype=np.uint8)
    for k, im in enumerate(images):
        r, c = divmod(k, columns)
        sheet[r * h:(r + 1) * h, c * w:(c + 1) * w] = im
    return sheet
