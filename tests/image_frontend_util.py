"""What the GPU tests of the image front end (test_gpu_klt.py, test_gpu_fast.py, test_gpu_orb.py, test_gpu_image_set_rule.py) share."""
import numpy as np


def as_hwc(img):
    img = np.asarray(img, np.uint8)
    return img[..., None] if img.ndim == 2 else img


def upload_images(imgs, padded):
    """(F, rows, cols[, 3]) uint8 on the device: dense, or a view into a block whose rows and frames are padded with 0xEE."""
    import torch
    dev = torch.device("cuda:0")
    a = np.stack([as_hwc(i) for i in imgs])
    n, rows, cols, cn = a.shape
    if not padded:
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    else:
        block = torch.full((n, rows + 3, cols + 5, cn), 0xEE, dtype=torch.uint8, device=dev)
        block[:, :rows, :cols] = torch.from_numpy(a).to(dev)
        t = block[:, :rows, :cols]
    return t[..., 0] if cn == 1 else t


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
