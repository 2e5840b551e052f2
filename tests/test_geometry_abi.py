"""CPU: ``msda_batch_geometry_f32`` (ABI v13, csrc/msda_geometry.h) refuses bad arguments on the host, before any launch, and says which call
refused; the ABI version is 13 in the header, the library and the binding; richsem_amd/geometry.py has no CPU fallback."""
import ctypes
import os
import re

import pytest
import torch

from richsem_amd import _build, _lib

from conftest import ROOT

NULL_POINTER, BAD_DIMS, MISALIGNED, TOO_LARGE = -1, -2, -5, -4
ARGS = ("sizes", "shapes", "mask_flat", "valid_ratios", "ref", "pos_sine", "proposals", "zeroed")


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def _call(lib, levels=((8, 12), (4, 6), (2, 3), (1, 2)), N=3, canvas=(64, 96), num_pos_feats=128, temperature=(20.0, 20.0), L=None, **ptrs):
    """the entry point with fake (never dereferenced) device pointers, 0x1000 unless given by name: every call below is refused on the host"""
    host = (ctypes.c_int32 * max(2 * len(levels), 1))(*[v for hw in levels for v in hw])
    p = {k: 0x1000 for k in ARGS}
    p["shapes"] = host
    p.update(ptrs)
    return lib.msda_batch_geometry_f32(p["sizes"], N, canvas[0], canvas[1], p["shapes"], len(levels) if L is None else L, num_pos_feats,
                                       temperature[0], temperature[1], p["mask_flat"], p["valid_ratios"], p["ref"], p["pos_sine"], p["proposals"],
                                       p["zeroed"], None)


def _refused(lib, code, **kw):
    seed = lib.msda_sine_embed_bf16(None, 4, 1, 4, 128, 10000.0, None, None)      # another call's text is in place ...
    assert seed < 0 and "msda_sine_embed_bf16" in _lib.last_error()
    assert _call(lib, **kw) == code, kw
    text = _lib.last_error()                                                      # ... and this call's own replaces it
    assert text.startswith("msda_batch_geometry_f32: "), text
    return text


def test_abi_version_is_13_everywhere(lib):
    header = open(os.path.join(ROOT, "include", "richsem_msda.h")).read()
    assert int(re.search(r"#define RICHSEM_MSDA_ABI_VERSION (\d+)", header).group(1)) == 13
    assert lib.msda_abi_version() == 13 and _lib.ABI_VERSION == 13
    assert "msda_batch_geometry_f32" in _lib.SYMBOLS and re.search(r"\bint msda_batch_geometry_f32\(", header)


@pytest.mark.parametrize("name", ["sizes", "shapes", "mask_flat", "valid_ratios"])
def test_a_required_pointer_may_not_be_null(lib, name):
    assert "null pointer" in _refused(lib, NULL_POINTER, **{name: None})


def test_proposals_and_zeroed_go_together(lib):
    assert "null pointer" in _refused(lib, NULL_POINTER, proposals=None)
    assert "null pointer" in _refused(lib, NULL_POINTER, zeroed=None)


@pytest.mark.parametrize("kw", [dict(L=0), dict(L=9, levels=((2, 2),) * 9), dict(levels=((8, 12), (0, 6))), dict(levels=((8, 12), (4, -1))),
                                dict(num_pos_feats=127), dict(num_pos_feats=1), dict(num_pos_feats=0), dict(num_pos_feats=258), dict(N=0),
                                dict(canvas=(0, 96)), dict(canvas=(64, 0)), dict(temperature=(0.0, 20.0)), dict(temperature=(20.0, -1.0))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items())[:40])
def test_dimensions_out_of_range_are_refused(lib, kw):
    assert "dimension" in _refused(lib, BAD_DIMS, **kw)


def test_misaligned_and_oversized_calls_are_refused(lib):
    for name, addr in (("sizes", 0x1002), ("valid_ratios", 0x1004), ("ref", 0x1004), ("pos_sine", 0x1008), ("proposals", 0x1008)):
        assert "aligned" in _refused(lib, MISALIGNED, **{name: addr}), name
    assert "too large" in _refused(lib, TOO_LARGE, levels=((1 << 15, 1 << 15), (1 << 15, 1 << 15)))      # N * S >= 2^31
    assert "too large" in _refused(lib, TOO_LARGE, levels=((1 << 16, 1 << 15),))                         # one level >= 2^31 pixels


def test_every_optional_output_may_be_null_and_the_checks_still_run(lib):
    """(the nullable outputs are not what refuses a call: with all of them null the next check -- here a bad level count -- still answers)"""
    assert "dimension" in _refused(lib, BAD_DIMS, ref=None, pos_sine=None, proposals=None, zeroed=None, L=0)


def test_python_layer_has_no_cpu_fallback_and_checks_its_arguments():
    import richsem_amd
    from richsem_amd import geometry
    assert richsem_amd.batch_geometry is geometry.batch_geometry and richsem_amd.sizes_from_targets is geometry.sizes_from_targets
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        geometry.batch_geometry(torch.tensor([[64, 96]], dtype=torch.int32), (64, 96))
    sizes = geometry.sizes_from_targets([{"size": torch.tensor([480.0, 640.0])}, {"size": torch.tensor([33, 47])}], "cpu")
    assert sizes.dtype == torch.int32 and sizes.tolist() == [[480, 640], [33, 47]]
    with pytest.raises(ValueError, match="size"):
        geometry.sizes_from_targets([{"size": torch.tensor([480.0])}], "cpu")


def test_the_entry_point_has_one_call_site():
    """the host-layer rule: a library entry point is called from one place in the Python package"""
    hits = []
    for d, _, files in os.walk(os.path.join(ROOT, "richsem_amd")):
        for f in files:
            if f.endswith(".py") and f != "_lib.py":
                text = open(os.path.join(d, f), encoding="utf-8").read()
                hits += [f] * len(re.findall(r"\.msda_batch_geometry_f32\(", text))
    assert hits == ["geometry.py"], hits
