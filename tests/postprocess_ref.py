"""The default route from a decoded value to a written pixel, restated once for tests/test_postprocess_cpu.py and tests/test_postprocess_gpu.py."""
import numpy as np


def quantise(v: np.ndarray) -> np.ndarray:
    """numpy fp32, every operation rounded on its own: torch.clamp((x + 1) / 2, 0, 1) (cli._finish), then the writers'
    (255.0 * .).astype(uint8) (video_io).  Defined for finite and infinite v; a NaN reaches numpy's float -> uint8 cast, whose result is
    unspecified, so callers keep NaN away from it."""
    f = np.float32
    y = np.minimum(np.maximum((v.astype(f) + f(1.0)) / f(2.0), f(0.0)), f(1.0))
    return (f(255.0) * y).astype(np.uint8)
