"""SHA-256 of the gfx950 assembly of every kernel source of the library (build.SOURCES compiled with build.FLAGS plus
--cuda-device-only -S), with the per-compile unit id (__hip_cuid_<hex>) replaced by a fixed token.  In the style of
tools/ops_binding_digests.py: run it in two trees and compare the output line by line -- a refactor of the kernel sources
that claims "same device code" must not move a line.  It hashes whole files and searches them for nothing.  Needs no GPU;
a file costs about 13 s to compile.

  python tools/device_asm_digests.py [--tree DIR] [--jobs N]     DIR: the tree whose recombiner_amd/csrc is compiled"""
import argparse
import hashlib
import importlib.util
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--jobs", type=int, default=8)
args = ap.parse_args()

spec = importlib.util.spec_from_file_location("rcb_build", os.path.join(os.path.abspath(args.tree), "recombiner_amd", "build.py"))
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)


def digest(src):
    cmd = [build.hipcc()] + build.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"]
    asm = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, cwd=build.CSRC).stdout   # (.file names the path as given)
    return hashlib.sha256(re.sub(rb"__hip_cuid_[0-9a-f]+", b"__hip_cuid_X", asm)).hexdigest()


with ThreadPoolExecutor(args.jobs) as ex:
    for src, d in zip(build.SOURCES, ex.map(digest, build.SOURCES)):
        print(f"{src:28s} {d}", flush=True)
