"""What tests/test_gpu_gla_grad.py, tests/test_gpu_misi_grad.py, tests/test_gpu_rtisi_grad.py and tests/test_gpu_windows_grad.py do
alike: moving arrays to the device and back, the per-spectrogram rows of a comparison, and the record of what a file's cases reached.
A plain module: no fixtures, nothing here is collected.  The checks, bars and caps are in the files themselves."""
import json
import os

import numpy as np

import gla_grad_cases


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cases are read-only)


def ptr(t):
    return None if t is None else t.data_ptr()


def f64(t):
    a = t.cpu().numpy()
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def rows_of(name, got, ref, per, seen=None):
    """(label, distance, bar) per spectrogram; seen: (B, T) bool, the frames compared, None for all."""
    rel = gla_grad_cases.rel
    pick = (lambda a, b: a[b]) if seen is None else (lambda a, b: a[b][seen[b]])
    return [("%s b=%d" % (name, b), rel(pick(got, b), pick(ref, b)), 3 * rel(pick(per, b), pick(ref, b))) for b in range(ref.shape[0])]


class Margins(dict):
    """Per shape key[:3] = (fsize, fshift, perfectrec), the figures named in `figures`: the count of whole-run rows first, then maxima."""

    def __init__(self, figures):
        super().__init__()
        self.figures = figures

    def row(self, key):
        return self.setdefault(key[:3], [0] + [0.0] * (len(self.figures) - 1))

    def note(self, key, rows=0, **figures):
        """Count `rows` whole-run rows and keep the largest of each figure, named as in `figures`, for the shape of `key`."""
        m = self.row(key)
        m[0] += rows
        for name, v in figures.items():
            m[self.figures.index(name)] = max(m[self.figures.index(name)], v)

    def report(self, filename):
        """The figures by name per shape, printed and written to $LWS_MARGINS_DIR/<filename> when that variable names a directory."""
        report = {"%d,%d,%s" % k: dict(zip(self.figures, v)) for k, v in sorted(self.items())}
        out = os.environ.get("LWS_MARGINS_DIR", "")
        if out and os.path.isdir(out):
            with open(os.path.join(out, filename), "w") as f:
                json.dump(report, f, indent=1)
                f.write("\n")
        print(report)
        return report
