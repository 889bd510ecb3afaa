"""Time streaming online MISI on the device (MisiLaStream, k_misi_la_stream of lws_gla.hip; look-ahead 3, 5 iterations, explicit
magnitudes, no signals) against the one-shot misi_la_dev on the same stack, for K = 2 and K = 4 sources:
  * the whole stack through misi_la_dev, alternating with a stream fed in chunks of T, 32, 4 and 1 frames (all pushes and finish();
    creating the stream, which allocates and synchronises, is outside the timed region);
  * one push of one frame (and its fshift mixture samples) into a stream in its steady state, at B = 1 and at B = 64: what a
    real-time caller waits for.  HIP events around the push give the device time, the wall clock from the call to the end of a
    synchronize what the caller sees.
HIP events, after a warm-up; medians and the spread over `--reps` alternating repetitions.
    PYTHONPATH=. python tools/time_misi_la_stream.py [--reps 9 --out profiles/misi_la_stream_iteration.json]"""
import argparse, json, time
import numpy as np, torch
import lws_amd

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--look-ahead", type=int, default=3)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_misi_la_stream.py needs a GPU")
fsize, fshift, B, T, CHUNKS, BS = (512, 128, 64, 500, [500, 32, 4, 1], [1, 64]) if not a.small else (64, 16, 3, 48, [48, 8, 4, 1], [1, 3])
LA, n = a.look_ahead, a.iters
F = fsize // 2 + 1
p = lws_amd.lws(fsize, fshift, perfectrec=True)
lo = fsize - fshift if fsize % fshift == 0 else fsize - fsize % fshift


def need(M):
    return 0 if M <= 0 else fshift * (M - 1) + fsize - lo


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median_ms": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def measure(K):
    g = torch.Generator(device="cuda"); g.manual_seed(K)
    length = lws_amd._capi.istft_length(T, fsize, fshift, True)
    x = torch.randn((B, K, length), device="cuda", generator=g)
    X = p.stft_dev(x.reshape(B * K, length)).reshape(B, K, T, F)
    c0 = X * torch.polar(torch.ones_like(X.real), 0.3 * torch.randn(X.shape, device="cuda", generator=g))
    A = X.abs()
    y = x.sum(dim=1)                                                     # what misi_la_dev takes
    yo = torch.cat([y, torch.zeros((B, need(T) - length), device="cuda")], dim=1)   # ... and a stream: the zeros stft pads with
    assert yo.shape[1] == need(T)

    def chunked(chunk):
        """The chunks as a caller would hold them: tensors of their own, cut outside the timed region."""
        parts = [(c0[:, :, at:at + chunk].contiguous(), yo[:, need(at):need(min(at + chunk, T))].contiguous(),
                  A[:, :, at:at + chunk].contiguous()) for at in range(0, T, chunk)]

        def run():
            s = p.misi_la_stream(K, n, look_ahead=LA, batch=B)
            ms = timed(lambda: [s.push(c, yy, m) for c, yy, m in parts] + [s.finish()])
            s.close()
            return ms
        return run

    runs = {"misi_la_dev": lambda: timed(lambda: p.misi_la_dev(c0, y, n, look_ahead=LA, magnitudes=A))}
    for chunk in CHUNKS:
        runs["stream_chunks_of_%d" % chunk] = chunked(chunk)
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):                      # alternate them
        for k, fn in runs.items():
            ms[k].append(fn())
    result = {"fsize": fsize, "fshift": fshift, "B": B, "K": K, "T": T, "iterations": n, "look_ahead": LA, "reps": a.reps,
              "whole_stack": {k: stats(v) for k, v in ms.items()}}
    one = result["whole_stack"]["misi_la_dev"]["median_ms"]
    for k in list(result["whole_stack"]):
        result["whole_stack"][k]["over_misi_la_dev_of_medians"] = result["whole_stack"][k]["median_ms"] / one
    result["one_commit_step_of_misi_la_dev_us"] = 1e3 * one / T

    # one push of one frame, steady state: streams of B = 1 and B = 64 primed with the first half of the stack, then a row at a time
    streams = {b: p.misi_la_stream(K, n, look_ahead=LA, batch=b) for b in BS}
    for b, s in streams.items():
        s.push(c0[:b, :, :T // 2].contiguous(), yo[:b, :need(T // 2)].contiguous(), A[:b, :, :T // 2].contiguous())
    rows = {b: [(c0[:b, :, m:m + 1].contiguous(), yo[:b, need(m):need(m + 1)].contiguous(), A[:b, :, m:m + 1].contiguous())
                for m in range(T // 2, T)] for b in BS}
    torch.cuda.synchronize()
    assert 2 * (a.warmup + a.reps) <= T - T // 2, "too many repetitions for the rows of the stack"
    dev, wall = {b: [] for b in BS}, {b: [] for b in BS}
    for rep in range(a.warmup + a.reps):
        for b, s in streams.items():             # alternate them
            c, yy, m = rows[b][2 * rep]
            d = timed(lambda: s.push(c, yy, m))
            c, yy, m = rows[b][2 * rep + 1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.push(c, yy, m)
            torch.cuda.synchronize()
            w = time.perf_counter() - t0
            if rep >= a.warmup:
                dev[b].append(d)
                wall[b].append(1e3 * w)
    for s in streams.values():
        s.close()
    result["push_of_one_frame"] = {"B=%d" % b: {"device_ms": stats(dev[b]), "call_to_synchronized_ms": stats(wall[b])} for b in BS}
    print(json.dumps(result), flush=True)
    return result


results = [measure(K) for K in (2, 4)]
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
        f.write("\n")
