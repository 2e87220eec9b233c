"""The host side of the SIREN kernels, pinned without a GPU: which descriptors the entry points accept (through the built
library, every data pointer NULL) and which kernel instance runs each accepted one (recombiner_amd/csrc/siren_route.h,
compiled alone by the host compiler with the address and undefined-behaviour sanitizers)."""
import hashlib
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _tool():
    spec = importlib.util.spec_from_file_location("siren_desc_digests", os.path.join(ROOT, "tools", "siren_desc_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _build(tmp, name, *defines):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp / name)
    # the sanitizer runtimes are linked into the program: it runs as it is, whatever else the loader brings along
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *defines]
    if "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx] + flags + [os.path.join(ROOT, "tests", "siren_route_sweep.cpp"), "-o", exe], check=True)
    return exe


def _run(*cmd):
    run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-2000:]      # (the program exits non-zero when one of its own assertions fails)
    return run.stdout


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """stdout of tests/siren_route_sweep.cpp and its "# " count lines"""
    out = _run(_build(tmp_path_factory.mktemp("siren_route"), "sweep"))
    tail = out[out.rindex(b"\n# descriptors ") + 1:].decode().splitlines()
    return out, [ln for ln in tail if ln.startswith("# ")]


def test_every_accepted_descriptor_has_one_route_and_the_routes_are_the_recorded_ones(sweep):
    with open(os.path.join(GOLDEN, "siren_routes.json")) as f:
        want = json.load(f)
    out, counts = sweep
    assert [ln[2:] for ln in counts] == want["counts"]
    assert hashlib.sha256(out).hexdigest() == want["sha256"]


def test_dealt32_build_routes_width_32_loss_and_backward_to_the_wide_family_on_request(tmp_path):
    """the descriptors beyond the lattice in a -DRCB_SIREN_DEALT32 build of the sweep: with dealt32 the width-32 loss / backward
    cases name the wide family's width-32 instances (or its refusal), forward and everything at dealt32 = 0 stay where they were"""
    with open(os.path.join(GOLDEN, "siren_routes.json")) as f:
        want = json.load(f)
    out = _run(_build(tmp_path, "sweep_dealt32", "-DRCB_SIREN_DEALT32"), "extras")
    lines = [ln for ln in out.decode().splitlines() if " p1 " in ln or " p2 " in ln]
    moved = [ln for ln in lines if "dealt32=1" in ln and " | m0 " not in ln and "rowwave" not in ln and "siren(deep)" not in ln
             and "siren(narrow)" not in ln]
    assert moved and all("-> wide(" in ln or "-> refused -3 siren(wide)" in ln for ln in moved)
    assert any(ln.endswith(",32) in16=1 dpe=0") for ln in moved)
    assert hashlib.sha256(out).hexdigest() == want["dealt32_extras_sha256"]


def test_route_sweep_and_library_accept_the_same_descriptors(sweep):
    with open(os.path.join(GOLDEN, "siren_desc_outcomes.json")) as f:
        want = json.load(f)
    head = sweep[1][0].split()
    for entry in ("rcb_siren_fwd", "rcb_siren_bwd", "rcb_siren_loss_bwd"):
        assert (int(head[2]), int(head[4])) == (want[entry]["descriptors"], want[entry]["accepted"]), entry


def test_library_answers_the_descriptor_lattice_as_recorded():
    import ctypes
    from recombiner_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "librcb_hip.so not built (python -m recombiner_amd.build)"
    with open(os.path.join(GOLDEN, "siren_desc_outcomes.json")) as f:
        want = json.load(f)
    got = _tool().run(ctypes.CDLL(_lib.LIB_PATH))
    for entry in _tool().ENTRIES:
        assert got[entry] == want[entry], entry
