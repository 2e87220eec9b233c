"""CPU tests of the product's host logic and of the C-ABI library surface (no GPU compute)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from golden_util import O, ROOT, cfg_of, check, load, prior_inputs, regen_noise

from recombiner_amd import _lib, config, ops, utils
from recombiner_amd import prior_model as PM


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "rcb.h")).read()
    declared = sorted(set(re.findall(r"\b(rcb_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 14
    assert os.path.exists(_lib.LIB_PATH), "librcb_hip.so not built (python -m recombiner_amd.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/rcb.h but not exported"
    assert sorted(_lib.EXPORTS) == declared
    assert _lib.load().rcb_version() == _lib.ABI_VERSION == int(re.search(r"#define RCB_VERSION (\d+)", hdr).group(1))


def test_descriptor_mirrors_have_the_library_sizes():
    """every ctypes mirror of a descriptor is as large as the structure the library was compiled with (rcb_struct_bytes) --
    _lib.load() refuses to bind otherwise -- and an unknown selector is rejected"""
    lib = _lib.load()
    for which, cls in _lib._MIRRORS.items():
        assert lib.rcb_struct_bytes(which) == ctypes.sizeof(cls), cls.__name__
    assert lib.rcb_struct_bytes(99) == -1


# ---------------------------------------------------------------------------------------------------
# the binding against the text of include/rcb.h: prototypes (_lib.PROTOTYPES) and structure fields (_lib._MIRRORS)
# ---------------------------------------------------------------------------------------------------
_C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
              "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double, "rcb_stream_t": ctypes.c_void_p}
_C_STRUCTS = {"rcb_siren_desc": _lib.SirenDesc, "rcb_level": _lib.Level, "rcb_level_bwd": _lib.LevelBwd,
              "rcb_adam_cfg": _lib.AdamCfg, "rcb_adam_tensor": _lib.AdamTensor, "rcb_rec_desc": _lib.RecDesc}


def _header():
    return open(os.path.join(ROOT, "include", "rcb.h")).read()


def _code_of(hdr):
    """the header without comments and preprocessor lines"""
    return re.sub(r"(?m)^\s*#.*$", "", re.sub(r"/\*.*?\*/|//[^\n]*", " ", hdr, flags=re.S))


def _ctype_of(ctype, in_struct):
    """the ctypes type the binding must use for a C type as the header spells it: every data pointer is c_void_p; a pointer
    to a descriptor as a PARAMETER is POINTER(mirror), const char* is c_char_p"""
    t = re.sub(r"\bconst\b", " ", ctype).replace("*", " * ").split()
    if "*" in t:
        if not in_struct and t == [t[0], "*"] and t[0] in _C_STRUCTS:
            return ctypes.POINTER(_C_STRUCTS[t[0]])
        return ctypes.c_char_p if t == ["char", "*"] else ctypes.c_void_p
    assert len(t) == 1 and t[0] in _C_SCALARS, f"C type {ctype!r} has no entry in the test's map"
    return _C_SCALARS[t[0]]


def _parse_prototypes(hdr):
    """[(name, return C type, [parameter C types])] of every rcb_*(...) declaration, in header order"""
    code = re.sub(r"typedef\b[^;{]*(\{.*?\})?[^;{]*;", "", _code_of(hdr), flags=re.S)           # structures, rcb_stream_t
    code = re.sub(r'extern\s+"C"\s*\{|\}', "", code)
    out = []
    for decl in (d.strip() for d in code.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(.+?)\b(rcb_[a-z0-9_]+)\s*\((.*)\)", decl, flags=re.S)
        assert m, f"cannot parse the declaration {decl!r}"
        params = [] if m.group(3).strip() == "void" else [p.strip() for p in m.group(3).split(",")]
        for p_ in params:
            assert re.fullmatch(r".*[\s*]\w+", p_, flags=re.S), f"{m.group(2)}: parameter {p_!r} has no name"
        out.append((m.group(2), m.group(1).strip(), [re.sub(r"\w+$", "", p_).strip() for p_ in params]))
    return out


def _parse_structs(hdr):
    """{structure name: [(field, C type, array length or None)]} of the typedef struct { ... } bodies; `int32_t rows, cols;`
    declares two fields, `int32_t v[3];` an array"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(rcb_\w+)\s*;", _code_of(hdr), flags=re.S):
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if not decl:
                continue
            m = re.fullmatch(r"(.*?[\s*])(\w+(?:\[\d+\])?(?:\s*,\s*\w+(?:\[\d+\])?)*)", decl, flags=re.S)
            assert m, f"{name}: cannot parse the member declaration {decl!r}"
            for item in m.group(2).split(","):
                f = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", item)
                fields.append((f.group(1), m.group(1).strip(), int(f.group(2)) if f.group(2) else None))
        out[name] = fields
    return out


def _prototype_mismatches(hdr, table):
    """what differs between the header's declarations and a name -> (restype, [argtypes]) table, each entry naming its function"""
    bad, declared = [], _parse_prototypes(hdr)
    names = [d[0] for d in declared]
    bad += [f"{n}: declared {names.count(n)} times" for n in sorted(set(names)) if names.count(n) > 1]
    bad += [f"{n}: declared in the header, not in the table" for n in names if n not in table]
    bad += [f"{n}: in the table, not declared in the header" for n in table if n not in names]
    if not bad and list(table) != names:
        bad.append("the table is not in header order: first difference at "
                   + next(a for a, b in zip(table, names) if a != b))
    for name, ret, params in declared:
        if name not in table:
            continue
        restype, argtypes = table[name]
        if restype is not _ctype_of(ret, False):
            bad.append(f"{name}: returns {ret}, the table says {restype.__name__}")
        if len(argtypes) != len(params):
            bad.append(f"{name}: {len(params)} parameters declared, {len(argtypes)} in the table")
            continue
        bad += [f"{name}: parameter {i} is {c}, the table says {a.__name__}"
                for i, (c, a) in enumerate(zip(params, argtypes)) if a is not _ctype_of(c, False)]
    return bad


def _struct_mismatches(hdr, mirrors):
    """what differs between the header's structures and {structure name: ctypes mirror}, each entry naming structure and field"""
    bad, structs = [], _parse_structs(hdr)
    if sorted(structs) != sorted(mirrors):
        bad.append(f"structures declared {sorted(structs)}, mirrored {sorted(mirrors)}")
    for name in sorted(set(structs) & set(mirrors)):
        want = [(f, _ctype_of(c, True), n) for f, c, n in structs[name]]
        have = [(f, getattr(t, "_type_", t), t._length_) if issubclass(t, ctypes.Array) else (f, t, None)
                for f, t in mirrors[name]._fields_]
        if [w[0] for w in want] != [h[0] for h in have]:
            k = next((i for i, (w, h) in enumerate(zip(want, have)) if w[0] != h[0]), min(len(want), len(have)))
            bad.append(f"{name}: field {k} is {want[k][0] if k < len(want) else None} in the header, "
                       f"{have[k][0] if k < len(have) else None} in the mirror ({len(want)} / {len(have)} fields)")
            continue
        bad += [f"{name}.{w[0]}: {w[1].__name__}{[w[2]] if w[2] else ''} in the header, {h[1].__name__}{[h[2]] if h[2] else ''} "
                "in the mirror" for w, h in zip(want, have) if w[1:] != h[1:]]
    return bad


def test_prototype_table_matches_the_header():
    """every rcb_*(...) declaration of include/rcb.h -- as many as the export test finds names -- has its return type and its
    parameter types, one by one and in header order, in _lib.PROTOTYPES, and the table has nothing else"""
    hdr = _header()
    declared = _parse_prototypes(hdr)
    assert len(declared) == len(set(re.findall(r"\b(rcb_[a-z0-9_]+)\s*\(", hdr))) == len(_lib.PROTOTYPES) >= 61
    assert _lib.EXPORTS == [d[0] for d in declared]
    assert _prototype_mismatches(hdr, _lib.PROTOTYPES) == []


def test_descriptor_mirrors_match_the_header_fields():
    """every ctypes mirror has the fields of its structure in include/rcb.h: names, order and types, comma declarators and
    arrays included; _lib._MIRRORS numbers them as the header's RCB_STRUCT_* selectors do"""
    hdr = _header()
    parsed = _parse_structs(hdr)
    assert len(parsed["rcb_level"]) == 13 and ("pe_patch_nums", "int32_t", 3) in parsed["rcb_siren_desc"]
    assert _struct_mismatches(hdr, _C_STRUCTS) == []
    selectors = {"rcb_" + n.lower(): int(v) for n, v in re.findall(r"#define RCB_STRUCT_(\w+) (\d+)", hdr)}
    assert {n: _lib._MIRRORS[v] for n, v in selectors.items()} == _C_STRUCTS


def _edited(hdr, old, new):
    assert hdr.count(old) == 1, old
    return hdr.replace(old, new)


def test_header_checks_report_drift():
    """the two comparisons fail, naming the function or the field, on copies of the header with one edit each"""
    hdr = _header()

    def protos(old, new):
        return _prototype_mismatches(_edited(hdr, old, new), _lib.PROTOTYPES)

    def structs(old, new):
        return _struct_mismatches(_edited(hdr, old, new), _C_STRUCTS)

    bad = protos("rcb_struct_bytes(int32_t which)", "rcb_struct_bytes(int64_t which)")            # a parameter widened
    assert len(bad) == 1 and bad[0].startswith("rcb_struct_bytes: parameter 0 is int64_t")
    bad = protos("float* scale, int64_t n, rcb_stream_t stream)", "float* scale, rcb_stream_t stream)")     # a parameter removed
    assert len(bad) == 1 and bad[0].startswith("rcb_softplus_scale: 3 parameters declared, 4 in the table")
    bad = protos("int rcb_version(void);", "int rcb_version(void);\nint rcb_new_entry(const float* x,\n  int32_t n);")
    assert bad == ["rcb_new_entry: declared in the header, not in the table"]                    # a declaration added
    bad = protos("int64_t rcb_stage1_1d_wgrad_workspace(void)", "int rcb_stage1_1d_wgrad_workspace(void)")
    assert len(bad) == 1 and bad[0].startswith("rcb_stage1_1d_wgrad_workspace: returns int,")    # a return type narrowed
    swapped = _edited(_edited(_edited(hdr, "float* g_loc;", "float* @;"), "float* g_log_scale;", "float* g_loc;"),
                      "float* @;", "float* g_log_scale;")                                        # two same-size fields swapped
    bad = _struct_mismatches(swapped, _C_STRUCTS)
    assert len(bad) == 1 and bad[0].startswith("rcb_level_bwd: field 20 is g_log_scale in the header, g_loc in the mirror")
    bad = structs("int32_t max_glen;", "uint32_t max_glen;")                                     # a field's signedness changed
    assert bad == ["rcb_rec_desc.max_glen: c_uint in the header, c_int in the mirror"]
    bad = structs("int32_t rows, cols, cols_out;", "int32_t rows, cols;  int64_t cols_out;")     # an int32 pair's neighbour widened
    assert len(bad) == 1 and bad[0].startswith("rcb_level.cols_out: c_long in the header")
    bad = structs("int32_t pe_patch_nums[3];", "int32_t pe_patch_nums[4];")                      # an array grown
    assert len(bad) == 1 and bad[0].startswith("rcb_siren_desc.pe_patch_nums:")
    table = dict(_lib.PROTOTYPES, rcb_not_in_header=(ctypes.c_int, []))
    assert _prototype_mismatches(hdr, table) == ["rcb_not_in_header: in the table, not declared in the header"]


def test_argument_classes_are_checked_at_the_call():
    """with the prototypes applied ctypes refuses, before the library is entered, an argument of the wrong class: a float or
    a pointer object for an integer parameter, another structure (or a plain integer) for a descriptor pointer, and too few
    arguments.  It does NOT refuse extra trailing arguments, nor an integer outside the parameter's range (the value is
    truncated to the declared width without a word): the wrappers in ops.py stay responsible for counts and ranges."""
    lib = _lib.load()
    for wrong in (1.0, ctypes.c_void_p(1)):
        with pytest.raises(ctypes.ArgumentError):
            lib.rcb_struct_bytes(wrong)
        with pytest.raises(ctypes.ArgumentError):
            lib.rcb_rec_workspace_bytes(4, wrong, 64)
    for wrong in (ctypes.byref(_lib.Level()), _lib.AdamCfg(), 4096):
        with pytest.raises(ctypes.ArgumentError):
            lib.rcb_step_tail_eligible(wrong)
    with pytest.raises(TypeError):
        lib.rcb_struct_bytes()
    with pytest.raises(TypeError):
        lib.rcb_rec_workspace_bytes(4, 3)
    assert lib.rcb_struct_bytes(99) == -1 and lib.rcb_struct_bytes(0) == ctypes.sizeof(_lib.SirenDesc)
    assert lib.rcb_rec_workspace_bytes(4, 3, 64) > 0 and isinstance(lib.rcb_last_error_string(), bytes)


def test_product_refuses_cpu_tensors():
    with pytest.raises(_lib.RcbError):
        ops.softplus_scale(torch.zeros(4))


def test_configs_match_reference_presets():
    for name in ("cifar", "protein"):
        assert config.configs[name] == cfg_of(load(f"prior_{name}.npz"))
    assert config.configs["kodak"]["hierarchical_patch_nums"] == {"level2": [4, 4], "level3": [8, 12]}
    assert config.configs["video"]["layerwise_scale_factors"] == [(6, 4, 4), 2, 2] or \
        config.configs["video"]["layerwise_scale_factors"] == [[6, 4, 4], 2, 2]
    assert config.configs["audio"]["patch_nums"] == [60]


def test_grouping_host_logic_exact():
    d = load("grouping.npz")
    names = ["group_idx", "start", "end", "group2param", "param2group", "n_groups", "group_kls", "weights"]
    for tag in "abc":
        r = PM.get_grouping_by_kl(d[f"{tag}_in"].copy())
        for k, v in zip(names, r):
            if k in ("group_kls", "weights"):
                np.testing.assert_allclose(np.asarray(v), d[f"{tag}_{k}"], rtol=1e-6)
            else:
                assert np.array_equal(np.asarray(v), d[f"{tag}_{k}"]), (tag, k)


def test_metrics_and_synthetic_inputs():
    d = load("metrics.npz")
    for ds in ["cifar", "kodak", "video", "audio", "protein"]:
        np.testing.assert_allclose(np.asarray(utils.metric(d["a"], d["b"], ds)), d["m_" + ds], rtol=1e-6)
    s = load("synthetic.npz")
    for name in ["cifar", "audio", "protein"]:
        X, Y = utils.synthetic_inputs(list(s[f"{name}_pixel_sizes"]), int(s[f"{name}_fourier_dim"]), 2, 3)
        np.testing.assert_allclose(X.numpy(), s[f"{name}_X"], atol=1e-6)
        assert Y.shape == (2, X.shape[0], 3) and float(Y.min()) >= 0 and float(Y.max()) < 1


@pytest.mark.parametrize("name", ["cifar", "protein", "patch2d", "patch1d", "patch3d"])
def test_patch_stitching_and_row_maps(name):
    d = load(f"prior_{name}.npz")
    cfg, geo, n, p, A, up, X, Y, pri = prior_inputs(d)
    eps = regen_noise(d, "fwd_eps")
    lpe = p["lpe_loc"] + O.st(p["lpe_log_scale"]) * eps[0]
    torch.manual_seed(124)
    net = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"])
    with torch.no_grad():
        pe = utils.map_lpe_to_inr_inputs(net, lpe[None], cfg["latent_dim"], cfg["pixel_sizes"], cfg["upsample_factors"],
                                         cfg["patch"], cfg["patch_nums"], cfg["data_dim"])[:, 0]
    check(d, "fwd_pe", pe, rtol=1e-5, atol=1e-6)
    if cfg["patch"]:
        m2, m3 = utils.hierarchy_row_maps(n, cfg["patch_nums"], cfg["hierarchical_patch_nums"], cfg["data_dim"])
        o2, o3 = geo.level_maps(n)
        assert np.array_equal(m2, o2.numpy()) and np.array_equal(m3, o3.numpy())


def test_level_spec_inverse_maps():
    rows, cols, n = 4, 7, 12
    rm = np.repeat(np.arange(rows), 3)
    perm = np.stack([np.random.RandomState(c).permutation(rows) for c in range(cols)], 1)
    cm = np.random.RandomState(1).permutation(cols)[:5]
    lv = ops.LevelSpec(torch.zeros(rows, cols), torch.zeros(rows, cols), 5, n, row_map=rm, row_perm=perm, col_map=cm)
    mp, mi = lv.member_ptr.numpy(), lv.member_idx.numpy()
    for r in range(rows):
        assert set(mi[mp[r]:mp[r + 1]]) == set(np.flatnonzero(rm == r))
    inv = lv.row_perm_inv.numpy()
    for j in range(cols):
        assert np.array_equal(perm[inv[:, j], j], np.arange(rows))
    ci = lv.col_inv.numpy()
    for dcol, j in enumerate(cm):
        assert ci[j] == dcol
    assert (ci[np.setdiff1d(np.arange(cols), cm)] >= 5).all()


# ---------------------------------------------------------------------------------------------------
# N4: bitstream container (pure host logic)
# ---------------------------------------------------------------------------------------------------
def test_bitstream_container_round_trip_and_rejects_corruption():
    from recombiner_amd import bitstream as B
    rng = np.random.RandomState(0)
    for shapes in ([(5, 7)], [(6, 11), (3, 4), (1, 9)], [(0, 3)], [(2, 0), (1, 1), (1, 1)]):
        levels = [rng.randint(0, 65536, size=s) for s in shapes]
        blob = B.pack_indices(levels)
        out = B.unpack_indices(blob)
        assert len(out) == len(levels) and all(np.array_equal(a, b) and b.dtype == np.int64 for a, b in zip(levels, out))
        n_idx = sum(int(np.prod(s)) for s in shapes)
        assert B.payload_bits(blob) == 16 * n_idx                      # 16 bits per (row, group): test_model.py:245-250
        assert len(blob) == 8 + 8 * len(shapes) + 2 * n_idx + 4        # header + indices + CRC, nothing else
    blob = B.pack_indices([np.array([[0, 65535, 258]])])
    assert blob[16:22] == bytes([0, 0, 255, 255, 2, 1])               # little-endian uint16
    bad = bytearray(blob)
    bad[17] ^= 1
    for broken in (bytes(bad), blob[:-1], blob + b"\0", b"XXXX" + blob[4:], blob[:4] + b"\x02\x00" + blob[6:]):
        with pytest.raises(ValueError):
            B.unpack_indices(broken)
    for a in (np.array([[65536]]), np.array([[-1]]), np.array([[1.5]]), np.array([1, 2, 3])):
        with pytest.raises(ValueError):
            B.pack_indices([a])
    with pytest.raises(ValueError):
        B.pack_indices([np.zeros((1, 1))] * 4)                          # at most three levels
    with pytest.raises(ValueError):
        B.unpack_indices(B.MAGIC + b"\x01\x00\x04\x10" + b"\0" * 40)   # header claiming four levels


def test_upsample_pickles_and_deep_copies_without_its_fast_path_caches():
    """the 16-bit modes cache their evaluation wrappers on the Upsample module; a checkpoint pickle (drivers.save_checkpoint
    writes the module itself, as main_prior_training.py:334-335 does) must stay loadable by the reference and a deep copy must
    not keep evaluating the original's parameters"""
    import copy
    import io
    import pickle
    from recombiner_amd import prior_model as PM
    from recombiner_amd.upsample_fast import phase_module, stitched2d_module
    net = PM.Upsample(2, [2, 1, 1], [4, 2, 2])
    assert phase_module(net) is not None and callable(stitched2d_module(net))
    assert any(k.startswith("_rcb_") for k in net.__dict__)
    blob = pickle.dumps(net)
    assert b"upsample_fast" not in blob and b"_rcb_" not in blob
    back = pickle.load(io.BytesIO(blob))
    assert not any(k.startswith("_rcb_") for k in back.__dict__)
    for a, b in zip(net.state_dict().values(), back.state_dict().values()):
        assert torch.equal(a, b)
    twin = copy.deepcopy(net)
    assert not any(k.startswith("_rcb_") for k in twin.__dict__)
    assert phase_module(twin).net is twin and phase_module(net).net is net


def test_bench_refuses_more_ranks_than_gpus():
    """`python bench.py --gpus N` starts N RCCL ranks itself; with fewer GPUs than ranks it must fail loudly instead of
    silently running one rank and printing n_gpus: 1 (no GPU call happens before the check: device_count() only)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RCB_DIST_BACKEND")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "64", "--steps", "1"], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--gpus 64 requested" in out.stderr and "{" not in out.stdout
    # a launcher that started a different number of ranks than --gpus says is refused as well
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1"],
                         env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "launcher started 1 rank" in out.stderr


def test_in_rank_capture_probe_decisions(monkeypatch):
    """bench.py under an external launcher (torchrun ... bench.py --gpus N): every rank probes the captured form of the sharded
    step in a CHILD process before it touches the GPU.  Host logic only: nothing is probed when the caller or bench.py's own
    launcher already chose, or on a gloo rehearsal; a probe that cannot run (here: no GPU for the child) selects the safe
    four-segment form instead of raising."""
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    sys.modules["bench_under_test"] = bench
    spec.loader.exec_module(bench)
    for k in ("RCB_CAPTURE_COLLECTIVES", "RCB_STEP_FORM_CHOICE", "RCB_DIST_BACKEND"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RCB_CAPTURE_COLLECTIVES", "0")
    assert bench.probe_capture_form_in_rank(2) is None
    monkeypatch.delenv("RCB_CAPTURE_COLLECTIVES")
    monkeypatch.setenv("RCB_STEP_FORM_CHOICE", "four segments (gloo rehearsal: no probe)")
    assert bench.probe_capture_form_in_rank(2) is None
    monkeypatch.delenv("RCB_STEP_FORM_CHOICE")
    monkeypatch.setenv("RCB_DIST_BACKEND", "gloo")
    assert bench.probe_capture_form_in_rank(2) is None
    monkeypatch.delenv("RCB_DIST_BACKEND")
    if not torch.cuda.is_available():                    # the child finds no GPU: exit code != 0 -> the safe form, no exception
        monkeypatch.setenv("RCB_PROBE_TIMEOUT_S", "120")
        monkeypatch.setenv("MASTER_PORT", "29931")
        assert bench.probe_capture_form_in_rank(1) is False


def test_reference_unpickles_a_checkpoint_written_by_the_product(tmp_path):
    """N2, product -> reference: a checkpoint written by drivers.save_checkpoint is read by the REFERENCE's own
    main_compression.py load sequence (eight plain pickle.load calls with the reference's prior_model on the path), the
    two modules come back as the reference's classes (without the product's fast-path caches), and the reference's
    TestBNNmodel built from them runs predict().  tests/golden/ckpt_ref_read.npz holds what the reference made of this very
    checkpoint (oracle/make_golden.py --only ckpt_read): the globals the file asked it to resolve and its predict() output.
    The file written here must ask for exactly those globals, carry no fast-path cache, and give the reference's predict()
    output again through the oracle's restatement of TestBNNmodel.predict."""
    import json
    import sys
    from golden_util import pickle_globals, product_checkpoint
    from recombiner_amd import drivers
    d = load("ckpt_ref_read.npz")
    ck, X = product_checkpoint()
    g1, lt, up = ck[0], ck[6], ck[7]
    path = os.path.join(tmp_path, "PRIOR.pkl")
    drivers.save_checkpoint(path, ck)
    assert PM.LinearTransform.__module__ == "recombiner_amd.prior_model" and "prior_model" not in sys.modules
    # the plain sequential pickle.load calls of main_compression.py:37-45, `prior_model.*` resolved to the product's classes
    # (the stand-ins of the reference's: same attribute, sub-module and parameter names)
    objs, names = pickle_globals(path, {"prior_model.LinearTransform": PM.LinearTransform, "prior_model.Upsample": PM.Upsample})
    assert len(objs) == 8
    assert names == json.loads(str(d["globals"])), (names, str(d["globals"]))
    assert "prior_model.LinearTransform" in names and "prior_model.Upsample" in names
    group_idx, gs, ge, g2p, p2g, n_groups, gk, w = objs[0]
    prior_loc, prior_scale, kl_beta, avg_ls = objs[1]
    linear_transform, upsample_net = objs[6], objs[7]
    assert type(linear_transform) is PM.LinearTransform and type(upsample_net) is PM.Upsample
    assert not any(k.startswith("_rcb_") for k in upsample_net.__dict__)
    assert n_groups == int(d["n_groups"])
    # the reference's predict() on what it read, restated by the oracle (test_model.py:283-320), on the same seed
    cfg = config.configs["cifar"]
    geo = O.Geometry.from_config(cfg)
    upo = O.UpsampleNet(geo.data_dim, geo.paddings, geo.layerwise_scale_factors)
    upo.weights = [q.detach().clone() for q in (upsample_net.conv1.weight, upsample_net.conv1.bias, upsample_net.conv2.weight,
                                                upsample_net.conv2.bias, upsample_net.conv3.weight, upsample_net.conv3.bias)]
    kw = dict(p_loc=prior_loc.clone()[p2g], p_log_scale=torch.log(torch.exp(prior_scale * 6) - 1).clone()[p2g],
              init_log_scale=avg_ls[p2g], group_idx=group_idx, group_start_index=gs, group_end_index=ge, group_to_param=g2p,
              n_groups=n_groups)
    tm = O.TestTimeModel(geo, 2, "cifar", [q.detach().clone() for q in linear_transform.A], upo, kw, initial_beta=kl_beta)
    with torch.no_grad():
        y = tm.predict(X[None].repeat(2, 1, 1), random_seed=3).numpy()
    y_ref = d["y_ref"]
    assert y_ref.shape == (2, 1024, 3) and np.isfinite(y_ref).all() and float(np.abs(y_ref).max()) > 0
    np.testing.assert_allclose(y, y_ref, rtol=1e-5, atol=1e-7)
    # and the same file read back by the product's loader gives the objects that were written
    back = drivers.load_checkpoint(path)
    assert all(torch.equal(a, b) for a, b in zip(back[6].A, lt.A)) and torch.equal(back[7].conv3.weight, up.conv3.weight)
    assert np.array_equal(back[0][4], g1[4]) and back[1][2] == 3e-7
