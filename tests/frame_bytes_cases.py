"""What tests/test_frame_bytes_cpu.py and tests/test_frame_bytes_gpu.py share: the two byte-frame laws as the reference computes them
(torch on the CPU) and the inputs at which a restatement of them can go wrong."""
import numpy as np
import torch


def unit_of_bytes(x):
    """uint8 -> fp32 in [0, 1] as minecraft/main2.py:51-56 does on the CPU."""
    return x.cpu().to(torch.float32).div(255)


def bytes_of_units(y):
    """save_image's law on a CPU tensor (any float dtype: taken to fp32 exactly first): mul(255).add_(0.5).clamp_(0, 255).to(uint8),
    with the one case torch leaves undefined -- NaN -- defined as 0."""
    t = y.cpu().float().mul(255).add_(0.5).clamp_(0, 255)
    return torch.where(t.isnan(), torch.zeros_like(t), t).to(torch.uint8)


def all_patterns(dtype):
    """Every one of the 65 536 bit patterns of a 16-bit float dtype, in order."""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).view(dtype)


def fp32_boundaries():
    """fp32 inputs around every rounding boundary of the law: k / 255 and (k +- 0.5) / 255 for every byte k, each with its two
    nextafter neighbours; then -0.0, negatives, values beyond 1, the largest and smallest magnitudes, +-inf and NaN."""
    k = np.arange(256, dtype=np.float32)
    centres = np.concatenate([k / np.float32(255), (k + np.float32(0.5)) / np.float32(255), (k - np.float32(0.5)) / np.float32(255)])
    up = np.nextafter(centres, np.float32(np.inf), dtype=np.float32)
    down = np.nextafter(centres, np.float32(-np.inf), dtype=np.float32)
    special = np.array([-0.0, 0.0, -1.0, -1e-8, -0.5 / 255, 1.0, 1.5, 2.0, 255.0, 256.0, 1e30, -1e30, 3.4028235e38, -3.4028235e38,
                        1e-45, -1e-45, 1.17549435e-38, np.inf, -np.inf, np.nan, -np.nan], dtype=np.float32)
    return torch.from_numpy(np.concatenate([centres, up, down, special]))
