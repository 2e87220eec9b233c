"""SHA-256 of what bitstream.py writes and of how it reads damaged streams, CPU only: run it in two trees and compare the output
line by line (a refactor of the container code must not move a byte, a parsed value or a refusal's text).

  python tools/bitstream_digests.py [--tree DIR] [--write FILE]
      DIR: the tree whose recombiner_amd is imported (default: this one); FILE: also write the lines as JSON {name: digest}
      (tests/golden/bitstream_outcomes.json is this file, and tests/test_ragged_emul_cpu.py holds the working tree to it)

pack    seeded index arrays of 1 and 3 levels through pack_indices: versions 1 to 4, extents of 1 to 3 axes, all four formats.
read    one small stream per version, and per mutation class -- intact, every other value of every single byte, every truncation --
        one digest over the outcomes of unpack, unpack_header and payload_bits each: the value returned, or the ValueError's text."""
import hashlib
import json
import os
import sys

import numpy as np

EXTENTS = {1: (37,), 2: (5, 7), 3: (3, 2, 9)}


def _sha(data):
    return hashlib.sha256(data if isinstance(data, bytes) else data.encode()).hexdigest()[:32]


def formats(SampleFormat):
    return [("u8", SampleFormat.u8()), ("f32", SampleFormat.f32()), ("u16_12", SampleFormat.u16(12)), ("s16", SampleFormat.s16())]


def levels(n_levels, seed=20):
    rng = np.random.RandomState(seed + n_levels)
    return [rng.randint(0, 1 << 16, size=shape) for shape in ((4, 5), (2, 3), (1, 7))[:n_levels]]


def pack_lines(bs, SampleFormat):
    for n_levels in (1, 3):
        lv = levels(n_levels)
        yield "pack v1 L%d" % n_levels, _sha(bs.pack_indices(lv))
        for nd, ext in EXTENTS.items():
            yield "pack v2 L%d nd%d" % (n_levels, nd), _sha(bs.pack_indices(lv, extent=ext))
        for name, fmt in formats(SampleFormat):
            yield "pack v3 L%d nd0 %s" % (n_levels, name), _sha(bs.pack_indices(lv, sample_format=fmt))
            for nd, ext in EXTENTS.items():
                yield "pack v3 L%d nd%d %s" % (n_levels, nd, name), _sha(bs.pack_indices(lv, extent=ext, sample_format=fmt))
                exts, swaps = [ext, tuple(v + 1 for v in ext)], [False, nd == 2]
                yield "pack v4 L%d nd%d %s" % (n_levels, nd, name), _sha(bs.pack_indices(lv, extents=exts, swaps=swaps, sample_format=fmt))


def streams(bs, SampleFormat):
    lv = [np.array([[1, 65535, 258], [0, 4660, 7]])]
    return {1: bs.pack_indices(lv), 2: bs.pack_indices(lv, extent=(5, 7)),
            3: bs.pack_indices(lv, extent=(5, 7), sample_format=SampleFormat.u16(12)),
            4: bs.pack_indices(lv, extents=[(5, 7), (6, 2)], swaps=[False, True], sample_format=SampleFormat.s16())}


def _show(v):
    if isinstance(v, np.ndarray):
        return "%s%s:%s" % (v.dtype.str, v.shape, _sha(np.ascontiguousarray(v).tobytes()))
    if isinstance(v, dict):
        return "{%s}" % ", ".join("%s=%s" % (k, _show(v[k])) for k in sorted(v))
    if isinstance(v, (list, tuple)):
        return "%s[%s]" % (type(v).__name__, ", ".join(_show(x) for x in v))
    return repr(v)


def outcome(fn, blob):
    try:
        return _show(fn(blob))
    except ValueError as e:
        return "ValueError: %s" % e


def mutations(blob):
    yield "intact", [blob]
    yield "byte", [blob[:i] + bytes([b]) + blob[i + 1:] for i in range(len(blob)) for b in range(256) if b != blob[i]]
    yield "truncation", [blob[:n] for n in range(len(blob))]


def read_lines(bs, SampleFormat):
    for version, blob in streams(bs, SampleFormat).items():
        for cls, blobs in mutations(blob):
            for fn in (bs.unpack, bs.unpack_header, bs.payload_bits):
                yield "read v%d %s %s" % (version, cls, fn.__name__), _sha("\n".join(outcome(fn, b) for b in blobs))


def lines(bs, SampleFormat):
    return list(pack_lines(bs, SampleFormat)) + list(read_lines(bs, SampleFormat))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--write", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from recombiner_amd import bitstream  # noqa: E402
    from recombiner_amd.utils import SampleFormat  # noqa: E402
    out = lines(bitstream, SampleFormat)
    for name, digest in out:
        print("%-40s %s" % (name, digest))
    if args.write:
        with open(args.write, "w") as f:
            json.dump(dict(out), f, indent=0, sort_keys=True)
            f.write("\n")
