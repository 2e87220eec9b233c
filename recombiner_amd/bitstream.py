"""N4: an auditable bitstream and a standalone decoder.

The reference writes the A* indices as a CSV of float-formatted numbers (main_compression.py:169-178) and has no
decoder: "decoding" is `predict` on the encoder's own object with every group masked.  Here the indices of all levels
are packed at ceil(log2 K) = 16 bits per (row, group) -- exactly the rate the reference's bpp formula charges
(test_model.py:245-250) -- and `decode()` rebuilds the signal from the prior checkpoint and the bitstream alone:

    z[row, start_g:end_g] = p_loc + p_scale * sobol_normal_table_g[idx[row, g]]      (test_model.py:501-533)

evaluated like the scoring kernel (fp64 multiply, then add, rounded to fp32 when committed), so the decoder's
parameters equal the encoder's bit for bit.

Container (little endian):  b"RCB1" | u16 version | u8 n_levels | u8 bits | per level: u32 rows, u32 n_groups |
payload: for each level (1, then 2 and 3 for patched presets) rows x n_groups uint16 indices, row-major | u32 CRC-32 of
the payload.

Version 2 (signals of any size, drivers.compress_signals_any): after the per-level shapes comes  u8 nd | nd x u32 size  -- the
signals' own extent per spatial axis; the model's grid is utils.fit_config(config, size), the signals were edge-padded to it and
`decode_signal_any` crops back -- and the CRC-32 covers that block and the payload, so a flipped size byte is rejected.  Rate of a
version-2 stream: bpp = payload_bits / (n_signals * prod(size)), bits per REAL sample position (the padding costs bits, it is not
counted as signal).

Version 3 (16-bit and other non-implied sample formats, utils.SampleFormat): the version-2 extent block -- here nd may be 0: the
signals fill the model's grid -- is followed by  u8 kind | u8 depth  (kind 0 u8, 1 f32, 2 u16 with depth 9 .. 16, 3 s16; depth 0
for all but u16), inside the CRC-32 like the extent.  It is written only when a format other than the preset's implied one (u8
for cifar / kodak / video, f32 for audio / protein) is given; versions 1 and 2 are byte for byte what they were.  The decoder
rounds to the format's lattice and can return the integers in its dtype.

Version 4 (signals of mixed sizes and orientations sharing one model, drivers.compress_signal_list): after the per-level shapes comes
u8 nd | u32 n_signals | n_signals x (nd x u32 size, u8 flags)  -- each signal's own extent along the MODEL's axes and its flags: bit
0 = "deliver with axes 0 and 1 exchanged" (2-D only: the signal was portrait and coded landscape), every other bit reserved and
rejected -- then  u8 kind | u8 depth, always present (the implied format is written out).  All sizes fit one grid
(utils.fit_config), and the level-1 rows are n_signals x the patches of that grid.  The CRC-32 of a version-4 stream covers the WHOLE
stream from the magic on, so a relabelled version number is caught as well; versions 1 to 3 stay byte for byte what they are.
`decode_signal_list` is its decoder.  Rate: bpp = payload_bits / sum of prod(size) over the signals."""
import struct
import typing
import zlib

import numpy as np
import torch

MAGIC = b"RCB1"
VERSION = 1
VERSION_EXTENT = 2
VERSION_FORMAT = 3
VERSION_LIST = 4


def _extent_block(extent):
    size = [int(v) for v in extent]
    if not 1 <= len(size) <= 3 or any(not 1 <= v <= 0xFFFFFFFF for v in size):
        raise ValueError("extent %r: 1 to 3 sizes in [1, 2^32) expected" % (tuple(extent),))
    return struct.pack("<B", len(size)) + struct.pack("<%dI" % len(size), *size)


def _format_block(sample_format):
    from .utils import SampleFormat
    if not isinstance(sample_format, SampleFormat):
        raise ValueError("sample_format %r: a utils.SampleFormat expected" % (sample_format,))
    return struct.pack("<BB", sample_format.kind, sample_format.depth)


def _list_block(extents, swaps, sample_format):
    extents = [[int(v) for v in e] for e in extents]
    swaps = [False] * len(extents) if swaps is None else [bool(v) for v in swaps]
    nd = len(extents[0]) if extents else 0
    if not 1 <= len(extents) <= 0xFFFFFFFF or not 1 <= nd <= 3 or len(swaps) != len(extents):
        raise ValueError("extents: a list of 1 to 2^32 - 1 sizes of 1 to 3 axes expected, and one swap flag for each")
    out = struct.pack("<BI", nd, len(extents))
    for size, sw in zip(extents, swaps):
        if len(size) != nd or any(not 1 <= v <= 0xFFFFFFFF for v in size):
            raise ValueError("extent %r: %d sizes in [1, 2^32) expected" % (tuple(size), nd))
        if sw and nd != 2:
            raise ValueError("only 2-D signals can be delivered with their axes exchanged")
        out += struct.pack("<%dIB" % nd, *size, 1 if sw else 0)
    return out + _format_block(sample_format)


def pack_indices(levels, bits=16, extent=None, sample_format=None, extents=None, swaps=None):
    """levels: list of integer arrays [rows, n_groups] with values < 2**bits  ->  bytes.  extent None: version 1; a tuple of the
    signals' size per spatial axis: version 2, which carries it.  sample_format (utils.SampleFormat): version 3, which carries
    the extent (or none: nd = 0) and the format.  extents (a list of sizes, one per signal; swaps: a flag for each, default
    none; sample_format required): version 4."""
    if bits != 16:
        raise ValueError("only 16 bits per group are defined (K = 65536 candidates, test_model.py:441-444)")
    if not 1 <= len(levels) <= 3:
        raise ValueError("1 to 3 levels expected")
    listed = extents is not None
    if listed and extent is not None:
        raise ValueError("extent and extents exclude each other")
    if not listed:                                           # (versions 1 to 3 refuse a bad extent before a bad index array)
        mid = b"" if extent is None else _extent_block(extent)
        version = VERSION if extent is None else VERSION_EXTENT
        if sample_format is not None:
            mid = (mid or struct.pack("<B", 0)) + _format_block(sample_format)
            version = VERSION_FORMAT
    shapes = body = b""
    for a in levels:
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError("index arrays must be [rows, n_groups]")
        if a.size and (a.min() < 0 or a.max() >= (1 << bits) or np.any(a != np.floor(a))):
            raise ValueError("index out of range for %d bits" % bits)
        shapes += struct.pack("<II", a.shape[0], a.shape[1])
        body += np.ascontiguousarray(a.astype("<u2")).tobytes()
    if listed:                                               # (version 4 after it)
        mid, version = _list_block(extents, swaps, sample_format), VERSION_LIST
    head = MAGIC + struct.pack("<HBB", version, len(levels), bits) + shapes
    covered = head + mid + body if listed else mid + body    # version 4: the checksum covers the whole stream
    return head + mid + body + struct.pack("<I", zlib.crc32(covered) & 0xFFFFFFFF)


class Stream(typing.NamedTuple):
    """A parsed and verified stream (_parse).  levels: the index arrays [rows, n_groups] as they lie in the stream (uint16 views,
    nothing converted); extent: the tuple a version-2 or -3 stream carries, else None; sample_format: the utils.SampleFormat a
    version-3 or -4 stream carries, else None; extents / swaps: a version-4 stream's per-signal sizes and exchange flags, else None."""
    version: int
    levels: list
    extent: typing.Optional[tuple]
    sample_format: object
    extents: typing.Optional[list]
    swaps: typing.Optional[list]

    def indices(self):
        return [a.astype(np.int64) for a in self.levels]


def unpack(blob):
    """bytes (any version) -> (list of int64 arrays [rows, n_groups], extent: the tuple a version-2 or -3 stream carries, None
    for version 1 and for a version-3 stream without one); raises ValueError on a malformed or corrupted stream.  The sample
    format of a version-3 stream: unpack_header."""
    s = _parse(blob)
    return s.indices(), s.extent


def unpack_header(blob):
    """bytes (any version) -> dict(version, extent, sample_format, extents, swaps): extent as `unpack` gives it, sample_format the
    utils.SampleFormat a version-3 or -4 stream carries (None for versions 1 and 2: the preset's implied format); a version-4
    stream adds extents / swaps, its per-signal sizes (tuples, along the model's axes) and exchange flags.
    Validates the whole stream as `unpack` does."""
    s = _parse(blob)
    names = ("version", "extent", "sample_format") + (("extents", "swaps") if s.version == VERSION_LIST else ())
    return {k: getattr(s, k) for k in names}


class _Cursor:
    """reads the header's fields in order; a field that the stream is too short for is a truncated header"""

    def __init__(self, blob, off):
        self.blob, self.off = blob, off

    def need(self, n_bytes):
        if self.off + n_bytes > len(self.blob):
            raise ValueError("truncated header")

    def take(self, fmt):
        self.need(struct.calcsize(fmt))
        out = struct.unpack_from(fmt, self.blob, self.off)
        self.off += struct.calcsize(fmt)
        return out


def _parse(blob):
    """bytes (any version) -> Stream; ValueError on a malformed or corrupted stream.  Every public function parses its stream once."""
    if len(blob) < 12 or blob[:4] != MAGIC:
        raise ValueError("not an RCB1 bitstream")
    version, n_levels, bits = struct.unpack_from("<HBB", blob, 4)
    if version not in (VERSION, VERSION_EXTENT, VERSION_FORMAT, VERSION_LIST) or bits != 16 or not 1 <= n_levels <= 3:
        raise ValueError("unsupported bitstream header (version %d, %d levels, %d bits)" % (version, n_levels, bits))
    cur = _Cursor(blob, 8)
    shapes = [cur.take("<II") for _ in range(n_levels)]
    start, extent, fmt, extents, swaps = cur.off, None, None, None, None
    if version == VERSION_LIST:
        nd, n_sig = cur.take("<BI")
        if not 1 <= nd <= 3 or n_sig < 1:
            raise ValueError("unsupported bitstream header (%d signals of %d axes)" % (n_sig, nd))
        cur.need(n_sig * (4 * nd + 1))
        extents, swaps = [], []
        for _ in range(n_sig):
            *size, flags = (int(v) for v in cur.take("<%dIB" % nd))
            if min(size) < 1:
                raise ValueError("bitstream extent %r has an empty axis" % (tuple(size),))
            if flags & ~1 or (flags and nd != 2):
                raise ValueError("unsupported bitstream header (signal flags 0x%02x for %d axes)" % (flags, nd))
            extents.append(tuple(size))
            swaps.append(bool(flags & 1))
        start = 0                                            # the checksum covers the whole stream
    if version in (VERSION_EXTENT, VERSION_FORMAT):
        (nd,) = cur.take("<B")
        if not (0 if version == VERSION_FORMAT else 1) <= nd <= 3:
            raise ValueError("unsupported bitstream header (an extent of %d axes)" % nd)
        if nd:
            extent = tuple(int(v) for v in cur.take("<%dI" % nd))
            if min(extent) < 1:
                raise ValueError("bitstream extent %r has an empty axis" % (extent,))
    if version in (VERSION_FORMAT, VERSION_LIST):
        from .utils import SampleFormat
        kind, depth = cur.take("<BB")
        try:
            fmt = SampleFormat(kind, depth)
        except ValueError as e:
            raise ValueError("unsupported bitstream header (%s)" % e) from None
    off = cur.off
    n_bytes = sum(r * g for r, g in shapes) * 2
    if len(blob) != off + n_bytes + 4:
        raise ValueError("bitstream length %d does not match its header (%d expected)" % (len(blob), off + n_bytes + 4))
    body = blob[off:off + n_bytes]
    (crc,) = struct.unpack_from("<I", blob, off + n_bytes)
    if zlib.crc32(blob[start:off + n_bytes]) & 0xFFFFFFFF != crc:
        raise ValueError("bitstream checksum mismatch")
    levels, p = [], 0
    for r, g in shapes:
        levels.append(np.frombuffer(body, dtype="<u2", count=r * g, offset=p).reshape(r, g))
        p += r * g * 2
    return Stream(version, levels, extent, fmt, extents, swaps)


def unpack_indices(blob):
    """bytes (any version) -> list of int64 arrays [rows, n_groups]; raises ValueError on a malformed or corrupted stream."""
    return _parse(blob).indices()


def payload_bits(blob):
    """bits spent on indices (what bpp is computed from; header and checksum are per-file constants)."""
    return sum(a.size for a in _parse(blob).levels) * 16


def _levels_of(model):
    return [model._l1] + ([model._l2, model._l3] if model.patch else [])


def encode(model, extent=None, sample_format=None, extents=None, swaps=None):
    """bitstream of a fully compressed TestBNNmodel (every group of every level encoded).  extent: the size of the signals
    when they were edge-padded to the model's grid (a version-2 stream, decode_signal_any); None: version 1, as ever.
    sample_format (utils.SampleFormat): a format other than the one the model's dataset implies makes it a version-3 stream that
    carries it; None or the implied format changes nothing.
    extents (one size per signal, along the model's axes; swaps: one flag per signal, default none): a version-4 stream, which
    always carries a format -- sample_format, or the implied one written out (decode_signal_list)."""
    from .utils import SampleFormat
    if extents is not None:
        extent = None                                        # (ignored beside extents, as ever)
        if sample_format is None:
            sample_format = SampleFormat.implied(model.dataset)
    elif sample_format is not None:
        if not isinstance(sample_format, SampleFormat):
            raise ValueError("sample_format %r: a utils.SampleFormat expected" % (sample_format,))
        if sample_format == SampleFormat.implied(model.dataset):
            sample_format = None
    lvls = _levels_of(model)
    for lv in lvls:
        if not lv.mask_groupwise.all():
            raise ValueError("level %r has %d groups that are not encoded yet" % (lv.pre, int((~lv.mask_groupwise).sum())))
    return pack_indices([lv.idx_groupwise for lv in lvls], extent=extent, sample_format=sample_format, extents=extents, swaps=swaps)


def apply_indices(model, levels):
    """Rebuild the encoded samples of every level of `model` from index arrays (decoder side): afterwards every group
    is marked encoded and `model.predict` reconstructs the signal."""
    from . import ops
    lvls = _levels_of(model)
    if len(levels) != len(lvls):
        raise ValueError("bitstream has %d levels, the model %d" % (len(levels), len(lvls)))
    K = int(np.ceil(2 ** model.bit_per_group))
    for lv, idx in zip(lvls, levels):
        if tuple(idx.shape) != (lv.rows, lv.n_groups):
            raise ValueError("level %r: index array %s, model needs %s" % (lv.pre, idx.shape, (lv.rows, lv.n_groups)))
        if idx.min() < 0 or idx.max() >= K:
            raise ValueError("level %r: index outside [0, %d)" % (lv.pre, K))
        dev = lv.loc.device
        tables = model._rec_tables(lv, lv.end - lv.start, K)
        # every (row, group) pair is one job of the encoder's own commit kernel (rcb_rec_commit): fp64 multiply, then add,
        # rounded to fp32 -- the decoder's parameters are the encoder's bit for bit by construction
        rows = np.repeat(np.arange(lv.rows), lv.n_groups)
        groups = np.tile(np.arange(lv.n_groups), lv.rows)
        jobs, order = ops.RecJobs.from_host(dev, rows, lv.start[groups], (lv.end - lv.start)[groups], group=groups,
                                            rows=lv.rows, cols=lv.D, sort=False)
        idx_t = torch.from_numpy(np.ascontiguousarray(idx.reshape(-1)).astype(np.int32)).to(dev)
        ops.rec_commit(lv.p_loc, ops.softplus_scale(lv.p_log_scale), tables, jobs, idx_t, n_groups=lv.n_groups,
                       enc_sample=lv.sample, enc_mask=lv.mask, done=lv.d_done, beta=lv.kl_beta, idx_groupwise=lv.d_idx)


def _decode_patches(config, dataset, checkpoint, stream, x, n_datapoints, device, seed, precision):
    from .drivers import build_test_model
    levels = stream.indices()
    if levels[0].shape[0] != n_datapoints:
        raise ValueError("bitstream holds %d rows, %d datapoints requested" % (levels[0].shape[0], n_datapoints))
    model = build_test_model(config, dataset, checkpoint, n_datapoints, device, seed)
    model.precision = precision
    apply_indices(model, levels)
    if x is None:
        from .utils import preset_inputs
        x = preset_inputs(config)
    with torch.no_grad():
        return model, model.predict(x.to(device))


def _try_parse(blob):
    """-> (Stream, None), or (None, the ValueError) for a decoder that has an older refusal to state first (_stream_format)"""
    try:
        return _parse(blob), None
    except ValueError as e:
        return None, e


def _stream_format(stream, error, dataset, sample_format, as_int):
    """the format the decoder rounds to: the one a version-3 or -4 stream carries, else `sample_format` (a version-1 / -2 stream
    whose caller knows it), else None -- the preset's implied format, through the code paths of versions 1 and 2.  ValueError when
    the two disagree, or when integers are asked of a format that has none.  stream None: the bytes did not parse, and `error`
    says why -- after the refusal that is older than the parser's."""
    from .utils import METRIC_ROUNDS
    if dataset not in METRIC_ROUNDS:
        raise ValueError(dataset)
    no_8bit = ValueError("%s signals have no 8-bit form (their metric does not round): decode them as fp32" % dataset)
    if stream is None:
        raise no_8bit if as_int and sample_format is None and not METRIC_ROUNDS[dataset] else error
    fmt = stream.sample_format
    if fmt is not None and sample_format is not None and fmt != sample_format:
        raise ValueError("the bitstream carries %r, sample_format says %r" % (fmt, sample_format))
    fmt = fmt if fmt is not None else sample_format
    if fmt is None and as_int and not METRIC_ROUNDS[dataset]:
        raise no_8bit
    if fmt is not None and as_int and not fmt.is_integer:
        raise ValueError("%r has no integer form: decode it as fp32" % (fmt,))
    return fmt


def _finish(y, dataset, fmt, as_int, layout, size=None):
    from . import ops
    from .utils import METRIC_ROUNDS
    mode = ops.RECON_8BIT if METRIC_ROUNDS[dataset] else ops.RECON_RAW
    q, whole, _, _ = ops.recon_finish(y.to(torch.float32).contiguous(), layout=layout, size=size, mode=mode, want_u8=as_int,
                                      want_whole=not as_int, sample_format=fmt)
    return q if as_int else whole


def decode(config, dataset, checkpoint, blob, x, n_datapoints, device="cuda", seed=42, precision=0, as_uint8=False,
           sample_format=None, as_integer=False):
    """Standalone decoder: prior checkpoint (drivers.load_checkpoint) + bitstream -> reconstruction [N, P, C].
    x: the coordinate features the encoder used ([P, F] or [N, P, F]; None: the preset's own, utils.preset_inputs(config));
    n_datapoints: INRs (patches) in the stream.
    as_uint8 (image / video presets): the 8-bit whole signals instead, uint8 [n_signals, *grid, C] with the patches of the
    patched presets stitched -- clip, x 255, round half to even, as the metric rounds (rcb_recon_finish).  audio / protein
    have no 8-bit form (their metric does not round): ValueError; `decode_signal` gives their fp32 whole signals.
    A version-2 stream is decoded like a version-1 stream: this is the patch level, `config` names the (fitted) grid and the
    result covers all of it, padding included; `decode_signal_any` crops to the size the stream carries.
    A version-3 stream likewise: the reconstruction [N, P, C] is not rounded at all; as_uint8 (alias: as_integer) gives the
    integers of the stream's format in its dtype (sample_format: the format of a version-1 / -2 stream, as decode_signal's)."""
    if as_uint8 or as_integer:
        stream, error = _try_parse(blob)
        fmt = _stream_format(stream, error, dataset, sample_format, True)
        return _decode_grid(config, dataset, checkpoint, stream, x, n_datapoints, device, seed, precision, True, fmt)
    return _decode_patches(config, dataset, checkpoint, _parse(blob), x, n_datapoints, device, seed, precision)[1]


def _decode_grid(config, dataset, checkpoint, stream, x, n_datapoints, device, seed, precision, as_int, fmt):
    # the whole GRID of `config`, for any version: `decode` is the patch-level decoder -- its caller names the (fitted) config
    # and the number of patches, and knows what the grid holds
    model, y = _decode_patches(config, dataset, checkpoint, stream, x, n_datapoints, device, seed, precision)
    return _finish(y, dataset, fmt, as_int, model.recon_layout())


def _refuse_list(stream, who):
    if stream is not None and stream.version == VERSION_LIST:
        raise ValueError("%s: a version-4 bitstream holds signals of their own sizes and orientations -- decode it with "
                         "decode_signal_list" % who)


def decode_signal(config, dataset, checkpoint, blob, x, n_datapoints, device="cuda", seed=42, precision=0, as_uint8=False,
                  sample_format=None, as_integer=False):
    """`decode`, finished on the device to WHOLE signals [n_signals, *grid, C] (n_signals = n_datapoints / patches per signal;
    [N, P, C] for the unpatched presets): fp32 -- on the 8-bit lattice k / 255 for the image / video presets, the raw values
    for audio / protein -- or, with as_uint8 (image / video only), the uint8 k themselves.
    A stream that carries an extent is refused (ValueError): its signals are smaller than the grid, decode_signal_any crops
    them back.
    sample_format (utils.SampleFormat): the format of a version-1 stream whose caller knows it (a version-3 stream carries its
    own; ValueError when they disagree): fp32 on the format's lattice, or with as_uint8 (alias: as_integer) the integers in
    the format's dtype -- uint16 for u16, int16 for s16."""
    as_uint8 = as_uint8 or as_integer
    stream, error = _try_parse(blob)
    _refuse_list(stream, "decode_signal")
    fmt = _stream_format(stream, error, dataset, sample_format, as_uint8)
    if stream.extent is not None:
        raise ValueError("a version-2 bitstream: its signals of size %r were edge-padded to the model's grid -- decode them with "
                         "decode_signal_any, which crops back (this decoder would return the padding)" % (stream.extent,))
    return _decode_grid(config, dataset, checkpoint, stream, x, n_datapoints, device, seed, precision, as_uint8, fmt)


def decode_signal_any(config, dataset, checkpoint, blob, device="cuda", seed=42, precision=0, as_uint8=False, as_integer=False):
    """The decoder of drivers.compress_signals_any: prior checkpoint + version-2 or -3 bitstream -> the signals [n, *size, C] at
    their own size.  `config` is the PRESET: the stream's extent fits it (utils.fit_config), the number of signals follows from the
    level-1 rows (ValueError when they are no whole number of signals), the patches are decoded with the preset's own coordinate
    features, and rcb_recon_finish_crop stitches, rounds (image / video presets) and crops on the device.  fp32 -- on the 8-bit
    lattice k / 255 for the image / video presets, raw for audio / protein -- or, with as_uint8 (image / video only), the k.
    A version-3 stream carries its sample format (unpack_header): the lattice is the format's (rcb_recon_finish_fmt), and
    as_integer (the clearer name of as_uint8) returns the integers in the format's dtype -- uint16 for u16, int16 for s16."""
    from . import ops
    from .utils import fit_config, preset_grid
    as_uint8 = as_uint8 or as_integer
    stream, error = _try_parse(blob)
    _refuse_list(stream, "decode_signal_any")
    fmt = _stream_format(stream, error, dataset, None, as_uint8)
    extent = stream.extent
    if extent is None:
        raise ValueError("a version-1 bitstream carries no signal size: decode it with decode_signal")
    if len(extent) != config["data_dim"]:
        raise ValueError("bitstream extent %r for a %d-D preset" % (extent, config["data_dim"]))
    fitted = fit_config(config, extent)
    pn, ps = preset_grid(fitted)
    per = int(np.prod(pn))
    rows = int(stream.levels[0].shape[0])
    if rows == 0 or rows % per:
        raise ValueError("bitstream holds %d rows, signals of size %r take %d patches each" % (rows, extent, per))
    _, y = _decode_patches(fitted, dataset, checkpoint, stream, None, rows, device, seed, precision)
    return _finish(y, dataset, fmt, as_uint8, ops.PeLayout(pn, ps), size=extent)


def decode_signal_list(config, dataset, checkpoint, blob, device="cuda", seed=42, precision=0, as_integer=False):
    """The decoder of drivers.compress_signal_list: prior checkpoint + version-4 bitstream -> the LIST of signals, each at its own
    size [*size_k, C] and in its own orientation (a signal flagged as exchanged comes back [size_k[1], size_k[0], C]: a portrait
    one portrait).  `config` is the PRESET: all sizes of the stream must fit one grid of it (utils.fit_config; ValueError
    otherwise, as when the level-1 rows are not n_signals x the patches of that grid), the patches are decoded with the preset's
    own coordinate features, and ONE rcb_recon_finish_ragged call stitches, rounds to the stream's sample format and crops every
    signal into its place.  fp32 on the format's lattice, or with as_integer the integers in the format's dtype (ValueError
    for f32, which has none)."""
    from . import ops
    from .utils import fit_config, preset_grid
    stream = _parse(blob)
    if stream.version != VERSION_LIST:
        raise ValueError("decode_signal_list: a version-%d bitstream -- decode it with decode_signal / decode_signal_any"
                         % stream.version)
    fmt = _stream_format(stream, None, dataset, None, as_integer)
    extents, swaps = stream.extents, stream.swaps
    dd = config["data_dim"]
    if len(extents[0]) != dd:
        raise ValueError("bitstream extents of %d axes for a %d-D preset" % (len(extents[0]), dd))
    fitted = fit_config(config, extents[0])
    pn, ps = preset_grid(fitted)
    for size in extents[1:]:
        if preset_grid(fit_config(config, size))[0] != pn:
            raise ValueError("bitstream extents %r and %r do not fit one grid of the preset" % (extents[0], size))
    per = int(np.prod(pn))
    rows = int(stream.levels[0].shape[0])
    if rows != len(extents) * per:
        raise ValueError("bitstream holds %d rows, %d signals take %d patches each" % (rows, len(extents), per))
    _, y = _decode_patches(fitted, dataset, checkpoint, stream, None, rows, device, seed, precision)
    q, whole, _, _ = ops.recon_finish_ragged(y.to(torch.float32).contiguous(), layout=ops.PeLayout(pn, ps), sizes=extents,
                                             swap=swaps, sample_format=fmt, want_int=as_integer, want_whole=not as_integer)
    return q if as_integer else whole
