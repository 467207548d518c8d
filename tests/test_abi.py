"""C-ABI surface checks that need no GPU: the library loads and exports every entry point
include/gcslam.h declares; the binding's header reader takes the subset of C the header uses and fails
loudly, naming the line, on anything else; argument errors map to ValueError."""

import os
import ctypes

import pytest

from gcslam import _abi, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gcslam.h")
LIB = os.path.join(ROOT, "fl-slam_amd", "gcslam", "libgcslam.so")


def declared():
    assert os.path.samefile(_header.HEADER_PATH, HEADER)
    return sorted(_header.load(HEADER)[0])


def test_header_declares_entries():
    names = declared()
    assert "gc_ctx_create" in names and "gc_scan_bins_fused" in names and "gc_iw_process_Q" in names
    assert len(names) >= 20


@pytest.mark.skipif(not os.path.exists(LIB), reason="libgcslam.so not built")
def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(LIB)
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


SNIPPET = """
/* a header in the manner of gcslam.h */
#define GC_OK 0
#define GC_ROW (484 + 22 + 16)   /* L, h, extras (16) */
#define GC_KEYS (1 << 23)
#define GC_TWO_ROWS (2 * GC_ROW - GC_OK)
#define GC_TAU_MIN 3e-3
#define GC_AT(B) ((B) + 1)
typedef struct gc_ctx gc_ctx;
struct gc_map; /* defined below */
typedef struct gc_map {
  int64_t m_slots;       /* (M), a comment; with a semicolon */
  int32_t n_lobes;
  const double* const weights;
  uint8_t** planes;
} gc_map;
typedef struct {
  float scale;
  uint64_t bytes;
} gc_dims;
int32_t gc_version(void);
const char* gc_last_error(const gc_ctx* ctx);
int32_t gc_update_Q(gc_ctx* ctx, const struct gc_map* map, /* the map (device), as gc_fuse(a, b) takes it */
                    const double* const d_in, void** d_out,
                    int64_t n, double eps,   // one, two
                    float gain, uint64_t bytes, const gc_dims* dims);
"""


def test_reader_takes_the_headers_subset():
    protos, structs, consts = _header.parse(SNIPPET)
    vp = ctypes.c_void_p
    assert protos == {
        "gc_version": ([], ctypes.c_int32),
        "gc_last_error": ([vp], ctypes.c_char_p),
        "gc_update_Q": ([vp, vp, vp, vp, ctypes.c_int64, ctypes.c_double, ctypes.c_float, ctypes.c_uint64, vp],
                        ctypes.c_int32)}
    assert consts == {"GC_OK": 0, "GC_ROW": 522, "GC_KEYS": 8388608, "GC_TWO_ROWS": 1044, "GC_TAU_MIN": 3e-3}
    assert "GC_AT" not in consts  # a function-like macro is skipped by rule
    assert type(consts["GC_KEYS"]) is int and type(consts["GC_TAU_MIN"]) is float
    assert sorted(structs) == ["gc_dims", "gc_map"]
    assert structs["gc_map"]._fields_ == [("m_slots", ctypes.c_int64), ("n_lobes", ctypes.c_int32), ("weights", vp),
                                          ("planes", vp)]
    assert structs["gc_dims"]._fields_ == [("scale", ctypes.c_float), ("bytes", ctypes.c_uint64)]
    assert issubclass(structs["gc_map"], ctypes.Structure) and ctypes.sizeof(structs["gc_map"]) == 8 + 4 + 4 + 8 + 8


@pytest.mark.parametrize("bad, line, word", [
    ("int32_t gc_f(gc_ctx* ctx,\n             size_t n);", 3, "size_t n"),                      # an unknown type token
    ("int32_t gc_f(unsigned int n);", 2, "unsigned int n"),
    ("typedef struct {\n  int64_t n;\n  double origin[3];\n} gc_s;", 4, "origin[3]"),        # an array member
    ("typedef struct {\n  gc_ctx ctx;\n} gc_s;", 3, "gc_ctx ctx"),                            # a struct by value
    ("typedef struct { int32_t n; } gc_s;\nint32_t gc_f(gc_s s);", 3, "gc_s s"),               # ... as an argument
    ("#define GC_A 1\n#define GC_B (GC_A / 2)", 3, "GC_B"),                                    # an operator outside the set
    ("#define GC_B (GC_LATER + 1)\n#define GC_LATER 1", 2, "GC_B"),                            # a name not defined yet
    ("#define GC_N sizeof(int)", 2, "GC_N"),
    ("#define GC_EMPTY", 2, "GC_EMPTY"),
    ("int32_t gc_ok(void);\nvoid gc_f(int32_t n);", 3, "gc_f"),                                # a return type it does not bind
    ("int32_t gc_f(int32_t (*cb)(int32_t));", 2, "gc_f"),                                      # a function pointer
])
def test_reader_fails_loudly(bad, line, word):
    text = "typedef struct gc_ctx gc_ctx;\n" + bad + "\n"
    with pytest.raises(RuntimeError) as e:
        _header.parse(text, "snippet.h")
    assert f"snippet.h:{line}:" in str(e.value) and word in str(e.value)
    assert text.split("\n")[line - 1].strip() in str(e.value)  # the offending line itself


def test_missing_header_is_a_runtime_error(tmp_path):
    with pytest.raises(RuntimeError, match="gcslam.h not found"):
        _header.load(str(tmp_path / "gcslam.h"))


def test_binding_is_the_headers():
    """What the package binds is what the reader yields from include/gcslam.h: every prototype with its
    restype, the constants as _abi.GC_*, the structs under the names the operators use."""
    protos, structs, consts = _header.load(HEADER)
    assert _abi.SIGNATURES == {n: a for n, (a, _) in protos.items()}
    assert _abi.PROTOTYPES["gc_last_error"] == ([ctypes.c_void_p], ctypes.c_char_p)
    assert all(r is ctypes.c_int32 for n, (_, r) in _abi.PROTOTYPES.items() if n != "gc_last_error")
    assert all(getattr(_abi, k) == v for k, v in consts.items()) and consts["GC_COMB_LEN"] == 550
    assert "GC_PCERT_MF" not in consts and not hasattr(_abi, "GC_PCERT_MF")
    assert len(_abi.GC_STAGE_NAMES) == _abi.GC_STAGE_N and len(_abi.GC_HS_NAMES) <= _abi.GC_HOST_STATS
    assert _abi.PipelineDims._fields_ == structs["gc_pipeline_dims"]._fields_
    assert len(structs) == 10 + len(CFG_BUILDERS)


def _cfg_builders():
    from gcslam import association, pipeline, primitive_map, rendering
    from gcslam.ops import camera_features, camera_splats, keypoint_detector, lidar_surfel_extraction
    mu = primitive_map.MapUpdateConfig()
    return dict(
        gc_pipeline_cfg=lambda: pipeline.PipelineConfig().as_struct(4),
        gc_map_update_cfg=lambda: _abi.cfg("gc_map_update_cfg", mu),
        gc_map_maintain_cfg=lambda: _abi.cfg("gc_map_maintain_cfg", mu),
        gc_ot_cfg=lambda: association._cfg(association.AssociationConfig(), 1e-9),
        gc_surfel_cfg=lambda: _abi.cfg("gc_surfel_cfg", lidar_surfel_extraction.SurfelExtractionConfig(), n_lobes=3),
        gc_cam_cfg=lambda: camera_splats._cfg(camera_splats.LidarCameraDepthFusionConfig()),
        gc_camfeat_cfg=lambda: camera_features._cfg(camera_features.VisualFeatureConfig()),
        gc_kp_cfg=lambda: keypoint_detector._cfg(keypoint_detector.OrbDetectorConfig()),
        gc_bev_cfg=lambda: rendering._bev_cfg(rendering.Viewport((0.0, 0.0), 8.0, 32, 32), rendering.SplatRenderingConfig(),
                                              0, 0.0),
        gc_camview_cfg=lambda: rendering._camview_cfg(rendering.CameraViewConfig()))


CFG_BUILDERS = _cfg_builders()


@pytest.mark.parametrize("name", list(CFG_BUILDERS))
def test_configuration_structs(name):
    """Every gc_*_cfg of the header is doubles only and unpadded, _abi.cfg builds it from exactly its member
    names, and the module that passes it fills every member from its default configuration."""
    st = _abi.STRUCTS[name]
    names = [n for n, _ in st._fields_]
    assert names and all(t is ctypes.c_double for _, t in st._fields_)
    assert ctypes.sizeof(st) == 8 * len(names)
    values = {n: float(i) for i, n in enumerate(names)}
    c = _abi.cfg(name, values)
    assert isinstance(c, st) and [getattr(c, n) for n in names] == list(values.values())
    with pytest.raises(TypeError, match=names[-1] + " is not given"):
        _abi.cfg(name, {n: v for n, v in values.items() if n != names[-1]})
    with pytest.raises(TypeError, match="no member no_such_member"):
        _abi.cfg(name, dict(values, no_such_member=1.0))
    built = CFG_BUILDERS[name]()
    assert isinstance(built, st) and all(getattr(built, n) == getattr(built, n) for n in names)  # filled, no NaN


def test_cfg_refuses_a_struct_that_is_not_all_double():
    with pytest.raises(TypeError, match="H_total is not a double"):
        _abi.cfg("gc_pipeline_dims", {n: 0 for n, _ in _abi.PipelineDims._fields_})


@pytest.mark.skipif(not os.path.exists(LIB), reason="libgcslam.so not built")
def test_version_and_null_ctx_errors():
    assert _abi.lib().gc_version() >= 10000
    with pytest.raises(ValueError):
        _abi.check(_abi.lib().gc_ctx_synchronize(None))


@pytest.mark.skipif(not os.path.exists(LIB), reason="libgcslam.so not built")
def test_packed_map_record_layout():
    """gc_primitive_map_record_layout (host-only): the fuse's read-modify-write fields in the first
    two 128-B lines of a 128-B-multiple record, no two fields overlapping, any lobe count; the Python
    map struct matches the header's field order and size."""
    import numpy as np
    from gcslam.primitive_map import _MapStruct
    widths = lambda L: [72, 24, 24 * L, 8, 8, 8, 8, 8, 8, 24, 8, 24, 24, 1, 8, 8]  # struct field order
    for L in range(1, 9):
        off = np.zeros(16, np.int64)
        sb = ctypes.c_int64(0)
        _abi.call("gc_primitive_map_record_layout", L, off.ctypes.data, ctypes.byref(sb))
        w = widths(L)
        spans = sorted((int(o), int(o) + w[k]) for k, o in enumerate(off))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (L, spans)
        assert sb.value % 128 == 0 and spans[-1][1] <= sb.value
        if L <= 3:  # Λ θ η w stamp seqs cam lidar accum denom: the first two lines
            assert max(int(off[k]) + w[k] for k in range(11)) <= 256
        # rgb and colors each own a whole 32-B sector (the fuse writes them as such)
        assert off[11] % 32 == 0 and off[12] % 32 == 0 and off[12] - off[11] >= 32
        assert all(not (off[11] < o < off[11] + 32 or off[12] < o < off[12] + 32) for o in off)
    with pytest.raises(ValueError):
        _abi.call("gc_primitive_map_record_layout", 9, off.ctypes.data, ctypes.byref(sb))
    # int64 m_slots, int32 n_lobes, int32 colors_current, 16 pointers, int64 slot_bytes
    assert ctypes.sizeof(_MapStruct) == 8 + 4 + 4 + 16 * 8 + 8
