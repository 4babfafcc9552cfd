"""CPU tests of the C-ABI boundary: the library loads without a GPU, exports every symbol that
include/gsplat/gs_abi.h declares, and fails loudly (error code + message) instead of falling back."""
import ctypes
import os
import re

import numpy as np
import pytest

from support import ROOT, c_layout, host_sources


def _declared():
    src = host_sources().hdr
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from gsplat import _abi
    L = _abi.load()
    names = _declared()
    assert "gs_create" in names and "gs_render" in names and len(names) >= 18
    for n in names:
        assert hasattr(L, n), "libgsplat_hip.so does not export %s" % n
    assert sorted(_abi.ABI_SYMBOLS) == names
    assert L.gs_abi_version() == 3


def test_struct_layouts_match_header(tmp_path):
    """The ctypes mirrors against what a C compiler makes of the header (sizeof / offsetof of every field)."""
    from gsplat import _abi
    assert ctypes.sizeof(_abi.GsConfig) == 48
    assert _abi.GsConfig.max_intersections.offset == 32 and _abi.GsConfig.stream.offset == 40
    fields = [n for n, _ in _abi.GsStats._fields_]
    prog = 'printf("%zu %zu", sizeof(gs_config), sizeof(gs_stats));'
    prog += "".join('printf(" %%zu", offsetof(gs_stats, %s));' % n for n in fields)
    out = c_layout(tmp_path, "layout", prog)
    assert out[0] == ctypes.sizeof(_abi.GsConfig) and out[1] == ctypes.sizeof(_abi.GsStats)
    assert out[2:] == [getattr(_abi.GsStats, n).offset for n in fields]


def test_header_documents_reference_interfaces():
    src = host_sources().hdr
    for cite in ("renderer.ts:96-102", "renderer.ts:349-593", "renderer.ts:130-137", "sort.ts:341-350",
                 "exclusive_scan.ts:208-325", "ply.ts:190-198", "process_gaussians.wgsl:8-15"):
        assert cite in src


def test_no_silent_fallback_without_gpu():
    """Without a HIP device gs_create must return an error code and a message -- never a CPU path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from gsplat import _abi
    import gsplat
    with pytest.raises(_abi.GsError) as e:
        gsplat.Renderer(gsplat.Canvas(64, 64), None, 0, gsplat.PackedGaussians(np.zeros((1, 80), np.float32)), 16)
    assert e.value.code in (-2, -3)
    L = _abi.load()
    cfg = _abi.GsConfig()
    cfg.struct_size = 7  # wrong size is rejected before anything else
    ctx = ctypes.c_void_p()
    assert L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)) == -1
    assert b"struct_size" in L.gs_last_error()
    assert L.gs_destroy(None) == 0


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gaussian-splatting-wgpu_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".js", ".hip", ".h", ".c", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "gs_oracle" not in txt and "np_oracle" not in txt and "oracle/" not in txt, os.path.join(dirpath, f)


# The public surface of gsplat's host classes: {class: {method: str(inspect.signature)}}, taken from the commit before
# PipelinedRenderer's forwards were generated.  One intended difference: the 25 owner calls, then written (*a, **kw), carry
# Renderer's exact signature.
PYTHON_HOST_SURFACE = {
    "Canvas": {"__init__": "(self, width, height)"},
    "PackedGaussians": {"__init__": "(self, records)", "from_ply": "(path)"},
    "InteractiveCamera": {"__init__": "(self, camera)", "setNewCamera": "(self, camera)", "isDirty": "(self)", "getCamera": "(self)"},
    "Renderer": {"__init__": "(self, canvas, interactiveCamera, device, gaussians, tileSize=16, *, flags=0, cols=None, max_intersections=0, "
            "stream=None, share_with=None)", "render_uniforms": "(self, uniforms, debug=False, out_ptr=None)", "animate": "(self, debug=False)",
        "wait": "(self)", "set_option": "(self, key, value)", "read_rgba8": "(self)", "read_buffer": "(self, which, dtype=<class 'numpy.uint32'>)",
        "read_alpha": "(self)", "read_depth": "(self, normalized=False)", "pick": "(self, xy, max_contrib=0)",
        "pick_rect": "(self, x0, y0, x1, y1, which='first')",
        "state_region": "(self, kind, op, bits, where=(0, 0), *, a=(0, 0, 0), b=(0, 0, 0), rect=(0, 0, 0, 0), uniforms=None, mask=None)",
        "state_ids": "(self, ids, op, bits)", "state_count": "(self, mask, value)", "read_state": "(self)", "write_state": "(self, arr)",
        "select_rect": "(self, x0, y0, x1, y1, uniforms, op=1)", "select_mask": "(self, mask, uniforms, op=1)",
        "select_sphere": "(self, centre, radius, op=1)", "select_box": "(self, lo, hi, op=1)", "clear_selection": "(self)",
        "hide_selected": "(self)", "unhide_all": "(self)", "accumulate_coverage": "(self, rect=None, mask=None)", "reset_coverage": "(self)",
        "read_coverage": "(self)", "state_coverage": "(self, op, bits, min_hits=1, min_weight=0.0, covered=True, where=(0, 0))",
        "select_visible": "(self, rect=None, mask=None, min_weight=0.0, op=1)", "hide_unseen": "(self, min_hits=1, min_weight=0.0)",
        "list_state": "(self, mask, value)", "export_splats": "(self, mask=0, value=0, with_ids=False, device=False)",
        "compact": "(self, mask, value)", "delete_hidden": "(self)", "save_ply": "(self, path, mask=0, value=0, sh_degree=3)",
        "transform": "(self, xform, mask=2, value=2)", "translate_selected": "(self, t)", "rotate_selected": "(self, rot, pivot=None)",
        "scale_selected": "(self, s, pivot=None)", "device_ptr": "(self, which)", "stats": "(self)",
        "assemble": "(self, d_slabs_ptr, col_bounds, slab_stride_bytes, d_image_ptr)", "destroy": "(self)"},
    "PipelinedRenderer": {"__init__": "(self, canvas, interactiveCamera, device, gaussians, tileSize=16, *, frames_in_flight=2, **kw)",
        "render_uniforms": "(self, uniforms)", "animate": "(self)", "wait": "(self, slot=None)", "read_rgba8": "(self, slot)",
        "read_alpha": "(self, slot)", "read_depth": "(self, slot, normalized=False)", "pick": "(self, slot, xy, max_contrib=0)",
        "set_option": "(self, key, value)",
        "state_region": "(self, kind, op, bits, where=(0, 0), *, a=(0, 0, 0), b=(0, 0, 0), rect=(0, 0, 0, 0), uniforms=None, mask=None)",
        "state_ids": "(self, ids, op, bits)", "state_count": "(self, mask, value)", "read_state": "(self)", "write_state": "(self, arr)",
        "select_rect": "(self, x0, y0, x1, y1, uniforms, op=1)", "select_mask": "(self, mask, uniforms, op=1)",
        "select_sphere": "(self, centre, radius, op=1)", "select_box": "(self, lo, hi, op=1)", "clear_selection": "(self)",
        "hide_selected": "(self)", "unhide_all": "(self)", "accumulate_coverage": "(self, rect=None, mask=None)", "reset_coverage": "(self)",
        "read_coverage": "(self)", "state_coverage": "(self, op, bits, min_hits=1, min_weight=0.0, covered=True, where=(0, 0))",
        "select_visible": "(self, rect=None, mask=None, min_weight=0.0, op=1)", "hide_unseen": "(self, min_hits=1, min_weight=0.0)",
        "list_state": "(self, mask, value)", "export_splats": "(self, mask=0, value=0, with_ids=False, device=False)",
        "save_ply": "(self, path, mask=0, value=0, sh_degree=3)", "transform": "(self, xform, mask=2, value=2)", "translate_selected": "(self, t)",
        "rotate_selected": "(self, rot, pivot=None)", "scale_selected": "(self, s, pivot=None)", "compact": "(self, mask, value)",
        "delete_hidden": "(self)", "destroy": "(self)"},
}


def test_python_host_surface():
    """Every public method of the host classes keeps its name and signature -- none missing, none added --, and a generated
    forward of PipelinedRenderer carries the docstring of the Renderer method it forwards to."""
    import inspect
    from gsplat import renderer
    live = {}
    for cname in PYTHON_HOST_SURFACE:
        cls = getattr(renderer, cname)
        live[cname] = {name: str(inspect.signature(getattr(cls, name))) for name in vars(cls)
                       if (name == "__init__" or not name.startswith("_")) and callable(getattr(cls, name))}
    assert live == PYTHON_HOST_SURFACE
    P, R = renderer.PipelinedRenderer, renderer.Renderer
    forwards = P._OWNER_CALLS + P._SLOT_CALLS
    assert len(P._OWNER_CALLS) == 25 and len(P._SLOT_CALLS) == 4 and len(set(forwards)) == 29
    for name in forwards:
        assert vars(P)[name].__doc__ == vars(R)[name].__doc__, name
        assert vars(P)[name] is not vars(R)[name]
    for name in P._OWNER_CALLS:
        assert PYTHON_HOST_SURFACE["PipelinedRenderer"][name] == PYTHON_HOST_SURFACE["Renderer"][name], name
