"""Compare two device assembly listings kernel by kernel: which functions have the same instruction stream (basic-block label
numbers and comments aside), which differ and where, and which exist in one listing only.  The way to check that a change to a
translation unit left its other kernels alone, e.g. for lws_gla.hip -- the unit: the file and the kernel headers it includes, lws_*_kernels.h,
lws_rtisi_march.h and lws_fft.h with its named transform instances (FFT_USER_*) -- against the parent commit:
    cd lws_amd/csrc
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S lws_gla.hip -o new.s
    git stash; hipcc ... -S lws_gla.hip -o old.s; git stash pop
    python ../../tools/compare_kernel_isa.py old.s new.s        (exit status 1 if a function of old.s differs or is gone)
"""
import difflib
import re
import sys


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\S+|[A-Za-z_]\w*):\s*; @", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        text = re.sub(r"\.LBB\d+_\d+", ".LBB", line.split(";")[0]).strip()
        if text:
            out[cur].append(text)
    return out


def main(old_path, new_path):
    old, new = functions(old_path), functions(new_path)
    bad = 0
    for name, body in old.items():
        if name not in new:
            print("GONE      %s" % name)
            bad += 1
        elif body == new[name]:
            print("same      %s (%d instructions and labels)" % (name, len(body)))
        else:
            print("DIFFERENT %s" % name)
            for d in list(difflib.unified_diff(body, new[name], lineterm="", n=1))[2:40]:
                print("    " + d)
            bad += 1
    for name in new:
        if name not in old:
            print("new       %s" % name)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
