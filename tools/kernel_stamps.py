"""What the *_stamps.py tools share: the diagnostic build of a stamp set (recombiner_amd/csrc/kernel_stamps.h), the library that
holds it, and the read-back of its array.  A tool calls select(SET) BEFORE it imports recombiner_amd, runs its workload, then
read(SET, shape).

    python tools/kernel_stamps.py            prints the build line of every set"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# set -> (variant name of the library, kernel source that holds the set)
SETS = {"SIREN": ("stamps", "siren_mlp_bf16.hip"), "WIDE": ("widestamps", "siren_mlp_wide.hip"), "WAVE": ("wstamps", "siren_mlp_wave.hip"),
        "ATRANS": ("atstamps", "atrans.hip"), "ATRANS_WG": ("atwgstamps", "atrans.hip"),
        "WC": ("wc", "upconv.hip"), "F2": ("f2", "upconv.hip"), "D2": ("d2", "upconv.hip"), "B3": ("b3", "upconv.hip")}


def library(name):
    return os.path.join(ROOT, "recombiner_amd", "lib", "librcb_%s.so" % SETS[name][0])


def build_line(name):
    variant, source = SETS[name]
    return "python -m recombiner_amd.build --variant %s --only %s -DRCB_STAMPS_%s=1" % (variant, source, name)


def select(name):
    """the tree on sys.path and the set's library in RCB_LIB (one named there already is kept)"""
    sys.path.insert(0, ROOT)
    lib = os.environ.setdefault("RCB_LIB", library(name))
    if not os.path.exists(lib):
        sys.exit("%s not found: %s" % (lib, build_line(name)))


def read(name, shape):
    """the set's array as int64 of the given shape"""
    try:
        entry = getattr(C.CDLL(os.environ["RCB_LIB"]), "rcb_debug_stamps_" + name)
    except AttributeError:
        sys.exit("not a stamps build: " + build_line(name))
    n = int(np.prod(shape))
    buf = (C.c_uint64 * n)()
    assert entry(buf, n) == 0
    return np.frombuffer(buf, dtype=np.uint64).astype(np.int64).reshape(shape)


if __name__ == "__main__":
    for name in SETS:
        print(build_line(name))
