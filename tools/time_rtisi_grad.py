"""Time training through RTISI-LA on the device at lws(512,128), T = 500 frames, look-ahead 3, n = 5 iterations, for B = 8 and
B = 256 spectrograms:
  rtisi_dev     lws_rtisi_la_dev, this build (and, with --parent-lib, another build of the library: the parent commit's)
  tape          lws_rtisi_la_tape_dev: the same march writing the tape
  backward      lws_rtisi_la_backward_dev from that tape, both cotangents, both gradients
and, on a clip of --clip frames (B = 8), what a training step pays against the alternative without this library:
  layer         rtisi_la_layer forward + loss.backward() through torch autograd
  torch         the same iteration written with torch ops (torch.fft, padding for the overlap-add) under torch autograd, forward +
                backward: thousands of small launches, which is why the clip is short
All variants of a row alternate in one process, in rotating order; HIP events around `--calls` calls, after a warm-up; medians and
the spread over `--reps`.
    PYTHONPATH=. python tools/time_rtisi_grad.py [--parent-lib path/to/liblws_hip.so] --out profiles/rtisi_grad_timing.json"""
import argparse, ctypes, json
import numpy as np, torch
import lws_amd

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--clip", type=int, default=24, help="frames of the clip the torch restatement runs on")
ap.add_argument("--parent-lib", action="append", default=[], help="another build of the library; may be given more than once")
ap.add_argument("--out", default=None)
ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_rtisi_grad.py needs a GPU")
fsize, fshift, T, LA, n = (512, 128, 500, 3, 5) if not a.small else (64, 16, 12, 3, 2)
BATCHES = (8, 256) if not a.small else (2, 3)
capi = lws_amd._capi
F = fsize // 2 + 1
p = lws_amd.lws(fsize, fshift)
aw, sw = (np.ascontiguousarray(w, dtype=np.float64) for w in (p.awin, p.swin))
vp, ci = ctypes.c_void_p, ctypes.c_int
libs = [("rtisi_dev", ctypes.CDLL(capi.LIB_PATH))]
libs += [("rtisi_dev_parent" + (str(i + 1) if i else ""), ctypes.CDLL(path)) for i, path in enumerate(a.parent_lib)]
for _, lib in libs:
    lib.lws_rtisi_la_dev.argtypes = [ci, vp, vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, vp]


def inputs(B, frames, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    length = capi.istft_length(frames, fsize, fshift, p.perfectrec)
    X = p.stft_dev(torch.randn((B, length), device="cuda", generator=g)).view(B, frames, F)
    A = X.abs()
    S = torch.polar(A, X.angle() + 0.1 * torch.randn(A.shape, device="cuda", generator=g))
    gC = (torch.randn(S.shape, device="cuda", generator=g) + 1j * torch.randn(S.shape, device="cuda", generator=g)).to(torch.complex64)
    gx = torch.randn((B, length), device="cuda", generator=g)
    return A, S, gC, gx, length


def measure(runs):
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms, names = {k: [] for k in runs}, list(runs)
    for r in range(a.reps):   # alternate the variants, each rep starting one further on
        for k in names[r % len(names):] + names[:r % len(names)]:
            ms[k].append(timed(runs[k]))
    return {k: {"median_ms": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in ms.items()}


def kernels_row(B):
    A, S, gC, gx, length = inputs(B, T, 1)
    C, x = torch.empty_like(S), torch.empty((B, length), dtype=torch.float32, device="cuda")
    tape = torch.empty((B, T, n, LA + 1, F), dtype=torch.complex64, device="cuda")
    gA, gS = torch.empty_like(A), torch.empty_like(S)

    def forward_of(lib):
        def f():
            C.copy_(S)
            rc = lib.lws_rtisi_la_dev(0, C.data_ptr(), A.data_ptr(), x.data_ptr(), B, T, fsize, fshift, aw.ctypes.data, sw.ctypes.data,
                                      int(p.perfectrec), n, LA, None)
            assert rc == 0
        return f

    def taped():
        C.copy_(S)
        capi.rtisi_la_tape_dev(C.data_ptr(), A.data_ptr(), x.data_ptr(), B, T, fsize, fshift, aw, sw, p.perfectrec, n, LA, tape.data_ptr())

    def backward():
        capi.rtisi_la_backward_dev(gC.data_ptr(), gx.data_ptr(), A.data_ptr(), tape.data_ptr(), B, T, fsize, fshift, aw, sw, p.perfectrec,
                                   n, LA, gA.data_ptr(), gS.data_ptr())

    runs = {name: forward_of(lib) for name, lib in libs}
    notes = {}
    runs["rtisi_dev"](); c1, x1 = C.clone(), x.clone()
    for name, _ in libs[1:]:   # the same seeded input, the same bits: the forward kernels are unchanged
        runs[name](); notes[name + "_same_bits"] = bool(torch.equal(C, c1) and torch.equal(x, x1))
    taped()   # the tape the timed backward reads
    notes["tape_same_bits"] = bool(torch.equal(C, c1) and torch.equal(x, x1))
    runs.update({"tape": taped, "backward": backward})
    row = {"fsize": fsize, "fshift": fshift, "B": B, "T": T, "look_ahead": LA, "iterations": n, "calls": a.calls, "reps": a.reps,
           "tape_bytes": tape.numel() * 8, "notes": notes}
    row.update(measure(runs))
    med = lambda k: row[k]["median_ms"]
    for name, _ in libs[1:]:
        row["rtisi_dev_over" + name[len("rtisi_dev"):]] = med("rtisi_dev") / med(name)
    row["tape_over_rtisi_dev"] = med("tape") / med("rtisi_dev")
    row["backward_over_tape"] = med("backward") / med("tape")
    return row


def torch_rtisi_la(A, S, win_a, win_s, keep, full):
    """lws_amd.rtisi_la(..., magnitudes=A, return_signal=True), start 'given', on a (B, T, F) stack with torch ops."""
    Tc = S.shape[1]
    place = lambda f, j: torch.nn.functional.pad(f, (fshift * j, full - fshift * j - fsize))
    inv = lambda c: torch.fft.irfft(c, n=fsize) * win_s
    c = [S[:, j] for j in range(Tc)]
    f = [inv(S[:, j]) for j in range(Tc)]
    done = torch.zeros((S.shape[0], full), device=S.device)
    for m in range(Tc):
        last = min(m + LA, Tc - 1)
        for _ in range(n):
            y = done
            for j in range(m, last + 1):
                y = y + place(f[j], j)
            y = y * keep
            for j in range(m, last + 1):
                X = torch.fft.rfft(y[:, fshift * j: fshift * j + fsize] * win_a)
                c[j] = A[:, j] * X / X.abs().clamp_min(1e-30)
            for j in range(m, last + 1):
                f[j] = inv(c[j])
        done = done + place(f[m], m)
    return torch.stack(c, dim=1), done * keep


def step_row(B, frames):
    A, S, gC, gx, length = inputs(B, frames, 2)
    leaves = [t.clone().requires_grad_(True) for t in (A, S)]
    win_a, win_s = (torch.from_numpy(w).float().cuda() for w in (aw, sw))
    full = fshift * (frames - 1) + fsize
    lo, hi = (fsize - (fsize % fshift or fshift), full - (fsize - fshift)) if p.perfectrec else (0, full)   # what istft cuts
    assert hi - lo == length
    keep = torch.zeros(full, device="cuda")
    keep[lo:hi] = 1.0

    def layer():
        for t in leaves:
            t.grad = None
        C, x = p.rtisi_la_layer(*leaves, n, look_ahead=LA, return_signal=True)
        ((gC.conj() * C).real.sum() + (gx * x).sum()).backward()

    def restated():
        for t in leaves:
            t.grad = None
        C, x = torch_rtisi_la(*leaves, win_a, win_s, keep, full)
        ((gC.conj() * C).real.sum() + (gx * x[:, lo:hi]).sum()).backward()

    runs, notes = {"layer": layer}, {}
    try:
        restated()
        g_torch = [t.grad.clone() for t in leaves]
        layer()
        torch.cuda.synchronize()
        notes["rel_l2_layer_to_torch_gA"] = float(((leaves[0].grad - g_torch[0]).norm() / g_torch[0].norm()).item())
        runs["torch"] = restated
    except Exception as e:   # reported, not hidden: the comparison is then "did not run"
        notes["torch"] = "did not run: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])
    row = {"fsize": fsize, "fshift": fshift, "B": B, "T": frames, "look_ahead": LA, "iterations": n, "calls": a.calls, "reps": a.reps,
           "notes": notes}
    row.update(measure(runs))
    if "torch" in runs:
        row["torch_over_layer"] = row["torch"]["median_ms"] / row["layer"]["median_ms"]
    return row


result = {"kernels": [kernels_row(B) for B in BATCHES], "training_step": step_row(BATCHES[0], a.clip if not a.small else 6)}
print(json.dumps(result), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "result": result}, f, indent=1)
        f.write("\n")
