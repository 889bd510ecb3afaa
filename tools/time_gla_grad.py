"""Time training through (Fast) Griffin-Lim on the device at lws(512,128), B = 8 spectrograms, T = 500 frames, n = 5 iterations,
alpha = 0.99:
  gla_dev       lws_griffin_lim_dev, this build (and, with --parent-lib, another build of the library: the parent commit's)
  tape          lws_griffin_lim_tape_dev: the same launches writing the tape
  backward      lws_griffin_lim_backward_dev from that tape, both gradients
  layer         griffin_lim_layer forward + loss.backward() through torch autograd (what a training step pays)
  torch         the alternative without this library: the iteration restated with torch.stft / torch.istft under autograd,
                forward + backward (its framing is torch's centred one, not this library's: the same work, not the same numbers)
All variants alternate in one process, in rotating order; HIP events around `--calls` calls, after a warm-up; medians and the spread over `--reps`.
    PYTHONPATH=. python tools/time_gla_grad.py [--parent-lib path/to/liblws_hip.so] --out profiles/gla_grad_timing.json"""
import argparse, ctypes, json
import numpy as np, torch
import lws_amd

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--parent-lib", action="append", default=[], help="another build of the library; may be given more than once")
ap.add_argument("--out", default=None)
ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_gla_grad.py needs a GPU")
fsize, fshift, B, T, n, alpha = (512, 128, 8, 500, 5, 0.99) if not a.small else (64, 16, 3, 12, 3, 0.99)
capi = lws_amd._capi
F = fsize // 2 + 1
p = lws_amd.lws(fsize, fshift)
g = torch.Generator(device="cuda"); g.manual_seed(1)
length = capi.istft_length(T, fsize, fshift, p.perfectrec)
src = torch.randn((B, length), device="cuda", generator=g)
X = p.stft_dev(src).view(B, T, F)
A = X.abs()
S = torch.polar(A, X.angle() + 0.1 * torch.randn(A.shape, device="cuda", generator=g))
aw, sw = (np.ascontiguousarray(w, dtype=np.float64) for w in (p.awin, p.swin))
C = torch.empty_like(S)
tape = torch.empty((n,) + tuple(S.shape), dtype=torch.complex64, device="cuda")
gA, gS = torch.empty_like(A), torch.empty_like(S)
gC = torch.randn(S.shape, device="cuda", generator=g) + 1j * torch.randn(S.shape, device="cuda", generator=g)
gC = gC.to(torch.complex64)
vp = ctypes.c_void_p


def forward_of(lib):
    lib.lws_griffin_lim_dev.argtypes = [ctypes.c_int] + [vp] * 2 + [ctypes.c_int] * 4 + [vp] * 2 + [ctypes.c_int] * 2 + [ctypes.c_double] + [vp] * 2

    def f():
        C.copy_(S)
        rc = lib.lws_griffin_lim_dev(0, C.data_ptr(), A.data_ptr(), B, T, fsize, fshift, aw.ctypes.data, sw.ctypes.data,
                                     int(p.perfectrec), n, alpha, None, None)
        assert rc == 0
    return f


def taped():
    C.copy_(S)
    capi.griffin_lim_tape_dev(C.data_ptr(), A.data_ptr(), B, T, fsize, fshift, aw, sw, p.perfectrec, n, alpha, tape.data_ptr())


def backward():
    capi.griffin_lim_backward_dev(gC.data_ptr(), A.data_ptr(), tape.data_ptr(), B, T, fsize, fshift, aw, sw, p.perfectrec, n, alpha,
                                  gA.data_ptr(), gS.data_ptr())


leaves = [t.clone().requires_grad_(True) for t in (A, S)]


def layer():
    for t in leaves:
        t.grad = None
    out = p.griffin_lim_layer(*leaves, n, alpha=alpha)
    (gC.conj() * out).real.sum().backward()


win_a, win_s = (torch.from_numpy(w).float().cuda() for w in (aw, sw))


def torch_restatement():
    for t in leaves:
        t.grad = None
    Tt = min(T, 1 + length // fshift)            # the frames torch's centred framing gives this length
    At, c = leaves[0][:, :Tt], leaves[1][:, :Tt]
    t_prev = None
    for i in range(1, n + 1):
        x = torch.istft(c.transpose(1, 2), fsize, hop_length=fshift, window=win_s, length=length)
        Xt = torch.stft(x, fsize, hop_length=fshift, window=win_a, return_complex=True).transpose(1, 2)[:, :Tt]
        t = At * Xt / Xt.abs().clamp_min(1e-30)
        c = t if i == 1 else t + alpha * (t - t_prev)
        t_prev = t
    (gC[:, :Tt].conj() * t_prev).real.sum().backward()


runs = {"gla_dev": forward_of(ctypes.CDLL(capi.LIB_PATH))}
parents = ["gla_dev_parent" + (str(i + 1) if i else "") for i in range(len(a.parent_lib))]
for name, path in zip(parents, a.parent_lib):
    runs[name] = forward_of(ctypes.CDLL(path))
runs.update({"tape": taped, "backward": backward, "layer": layer})
notes = {}
try:
    torch_restatement()
    torch.cuda.synchronize()
    runs["torch"] = torch_restatement
except Exception as e:   # reported, not hidden: the comparison is then "did not run"
    notes["torch"] = "did not run: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.calls


runs["gla_dev"](); c1 = C.clone()
for name in parents:   # the same seeded input, the same bits: the forward kernels are unchanged
    runs[name](); notes[name + "_same_bits"] = bool(torch.equal(C, c1))
taped()   # the tape the timed backward reads
notes["tape_same_bits"] = bool(torch.equal(C, c1))
for _ in range(a.warmup):
    for fn in runs.values():
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in runs}
names = list(runs)
for r in range(a.reps):   # alternate the variants, each rep starting one further on: what a variant follows costs it a few per cent
    for k in names[r % len(names):] + names[:r % len(names)]:
        ms[k].append(timed(runs[k]))
row = {"fsize": fsize, "fshift": fshift, "B": B, "T": T, "iterations": n, "alpha": alpha, "calls": a.calls, "reps": a.reps,
       "tape_bytes": tape.numel() * 8, "notes": notes}
for k, v in ms.items():
    row[k] = {"median_ms": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
med = lambda k: row[k]["median_ms"]
for name in parents:
    row["gla_dev_over" + name[len("gla_dev"):]] = med("gla_dev") / med(name)
row["tape_over_gla_dev"] = med("tape") / med("gla_dev")
row["backward_over_tape"] = med("backward") / med("tape")
row["layer_over_tape_plus_backward"] = med("layer") / (med("tape") + med("backward"))
if "torch" in runs:
    row["torch_over_layer"] = med("torch") / med("layer")
print(json.dumps(row), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "result": row}, f, indent=1)
        f.write("\n")
