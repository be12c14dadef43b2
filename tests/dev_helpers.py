"""Device memory of the GPU tests that call the `_dev` entry points directly (no torch): arrays that live as long as one test."""
import numpy as np


class Dev:
    """device arrays of one test, freed at its end"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, a) -> int:
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        p = self.ctx.dev_malloc(max(a.size, 16))
        self.ptrs.append(p)
        if a.size:
            self.ctx.dev_upload(p, a)
        return p

    def alloc(self, n) -> int:
        p = self.ctx.dev_malloc(max(n, 16))
        self.ptrs.append(p)
        return p

    def get(self, p, n):
        self.ctx.synchronize()
        return self.ctx.dev_download(p, n)

    def close(self):
        self.ctx.synchronize()
        for p in self.ptrs:
            self.ctx.dev_free(p)


def record_to_affine(rec):
    """68-byte record -> the 64 bytes mina_msm returns (zeros at infinity)"""
    rec = np.asarray(rec, np.uint8)
    return np.zeros(64, np.uint8) if rec[64:68].any() else rec[:64].copy()
