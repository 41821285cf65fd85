"""not-gpu: the C-ABI library loads on a GPU-less host and exports every symbol that
include/uda_clr_hip.h declares (no compute calls here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "uda_clr_amd", "lib", "libuda_clr_hip.so")


def _declared():
    txt = open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(uda_[a-z0-9_]+)\s*\(", txt)))


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_library_exports_every_declared_symbol():
    from uda_clr_amd.kernels import SYMBOLS, load_library
    lib = load_library()
    declared = _declared()
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), "missing export: " + name
    assert set(declared) == set(SYMBOLS), (set(declared) ^ set(SYMBOLS))
    assert lib.uda_version() >= 3      # 2: the depthwise entries take `family`; 3: uda_upconv_fwd accumulates stats for every geometry
    assert lib.uda_last_error() is not None


def _header():
    return open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()


def test_names_read_by_abi_are_the_declared_ones():
    """two independent readers of the header: the regex above and uda_clr_amd.abi"""
    from uda_clr_amd import abi
    assert sorted(abi.SYMBOLS) == _declared() and len(abi.SYMBOLS) >= 118


def test_header_is_read_completely():
    """read_header raises on anything it does not understand, so returning at all means no residue; the three argument blocks have
    the sizes the C compiler gives them and every signature consists of ctypes types a function pointer accepts"""
    import ctypes as C
    from uda_clr_amd import abi
    constants, structs, symbols = abi.read_header(_header())
    assert {n: C.sizeof(s) for n, s in structs.items()} == {"uda_src_t": 80, "uda_conv_args_t": 192, "uda_wgrad_args_t": 160}
    assert [f for f, _ in structs["uda_src_t"]._fields_] == ["x", "ldx", "N", "H", "W", "C", "scale", "shift", "act", "_pad", "mask",
                                                              "ldm", "mask_scale", "_pad2"]
    assert structs["uda_conv_args_t"].src.offset == 0 and structs["uda_conv_args_t"].w.offset == 80       # nested by value
    assert len(symbols) == len(abi.SYMBOLS) >= 118 and constants == abi.CONSTANTS
    proto = C.CFUNCTYPE(None)
    for name, (res, args) in symbols.items():
        fn = proto()
        fn.restype, fn.argtypes = res, args            # what load_library does; TypeError for anything that is no ctypes type
        assert all(hasattr(t, "from_param") for t in args), name
    assert symbols["uda_last_error"] == (C.c_char_p, []) and symbols["uda_version"] == (C.c_int, [])
    conv = symbols["uda_conv_route"]
    assert conv[1][0]._type_ is structs["uda_conv_args_t"] and conv[1][1:] == [C.c_char_p, C.c_int]
    assert symbols["uda_x3_packed_bytes"] == (C.c_uint64, [C.c_int64, C.c_int])
    assert symbols["uda_tta_fuse"][1][:5] == [C.c_void_p] * 4 + [C.c_int]


@pytest.mark.parametrize("what, old, new, named", [
    ("unknown parameter type", "int uda_relayout_dw(const float* w, int C,", "int uda_relayout_dw(const float* w, unsigned C,", "uda_relayout_dw"),
    ("unknown return type", "int uda_version(void);", "void uda_version(void);", "uda_version"),
    ("unterminated prototype", "int uda_version(void);", "int uda_version(void)", "uda_version"),
    ("unterminated last prototype", "int pre_op, float* d_logits_nchw, void* stream);", "int pre_op, float* d_logits_nchw, void* stream)",
     "uda_adv_s2d_bwd"),
    ("stray token between two declarations", "int uda_version(void);", "int uda_version(void);\nstray", "stray"),
    ("stray token before a typedef", "typedef struct uda_conv_args {", "stray typedef struct uda_conv_args {", "stray"),
    ("unknown member type", "int32_t act; ", "short act; ", "uda_src"),
])
def test_bad_header_raises_and_names_the_declaration(what, old, new, named):
    from uda_clr_amd import abi
    txt = _header()
    assert txt.count(old) == 1, what
    with pytest.raises(ValueError, match=named):
        abi.read_header(txt.replace(old, new))


def test_constants_are_the_headers():
    from uda_clr_amd import abi, acts
    names = ["UDA_STAT_SLOTS", "UDA_ACT_NONE", "UDA_ACT_RELU", "UDA_ACT_RELU6", "UDA_MFMA_F32", "UDA_MFMA_BF16X3", "UDA_DW_AUTO",
             "UDA_DW_FLAT", "UDA_DW_TILED", "UDA_DW_CB", "UDA_DW_FWD", "UDA_DW_DGRAD", "UDA_DW_WGRAD"]
    assert all(isinstance(abi.CONSTANTS.get(n), int) for n in names), abi.CONSTANTS
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert abi.CONSTANTS == {n: int(v) for n, v in re.findall(r"#define\s+(UDA_\w+)\s+(-?\d+)\s*$", txt, flags=re.M)}
    assert (acts.ACT_NONE, acts.ACT_RELU, acts.ACT_RELU6) == tuple(abi.CONSTANTS["UDA_ACT_" + a] for a in ("NONE", "RELU", "RELU6"))
    from uda_clr_amd import kernels
    assert kernels.STAT_SLOTS == abi.CONSTANTS["UDA_STAT_SLOTS"]
    assert (kernels.HipKernels.MFMA_F32, kernels.HipKernels.MFMA_BF16X3) == (abi.CONSTANTS["UDA_MFMA_F32"], abi.CONSTANTS["UDA_MFMA_BF16X3"])
    assert kernels._DW_FAMILY == {"": abi.CONSTANTS["UDA_DW_AUTO"], "flat": abi.CONSTANTS["UDA_DW_FLAT"],
                                  "tiled": abi.CONSTANTS["UDA_DW_TILED"], "cb": abi.CONSTANTS["UDA_DW_CB"]}
    assert kernels._DW_OP == {"fwd": abi.CONSTANTS["UDA_DW_FWD"], "dgrad": abi.CONSTANTS["UDA_DW_DGRAD"], "wgrad": abi.CONSTANTS["UDA_DW_WGRAD"]}
    assert (kernels.UdaSrc, kernels.UdaConvArgs, kernels.UdaWgradArgs) == tuple(
        abi.STRUCTS[n] for n in ("uda_src_t", "uda_conv_args_t", "uda_wgrad_args_t")) and kernels.SYMBOLS is abi.SYMBOLS


def test_header_cites_reference_lines():
    txt = open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()
    for anchor in ("mobilenet.py", "aspp.py", "decoder.py", "Trainer_prototype_full.py", "utils/Utils.py", "utils/metrics.py"):
        assert anchor in txt
