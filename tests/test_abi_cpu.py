"""The binding is read from include/egc_hip.h (egc_amd/_abi.py).  Two parts: answers spelled here BY HAND
from the header's text, which the reader must reproduce (so that it cannot degrade to "everything is a pointer"), and its
strictness on snippets: what it does not understand raises and names the text.  Then the one reading of an on/off switch, in
C++ (tests/env_on) and in Python."""
import ctypes as C
import os
import subprocess

import pytest

from egc_amd import _C, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L, F, D, Z = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t
LETTERS = {"P": P, "i": I, "l": L, "f": F, "d": D, "z": Z}


def spelled(letters):
    return [LETTERS[ch] for ch in letters.replace(" ", "")]


def test_argument_lists_spelled_by_hand():
    assert _C.SYMBOLS["egc_nbr_sum_f32"] == (C.c_int, spelled("PP lll Pi Pi iii f PPPPP Pi Pz P"))
    assert len(_C.SYMBOLS["egc_nbr_sum_f32"][1]) == 23
    assert _C.SYMBOLS["egc_pna_scale_combine_f32"] == (C.c_int, spelled("Pl Pi dd i Pi Pi Pi P"))
    assert _C.SYMBOLS["egc_gat_backward_dropout_f32"] == (C.c_int, spelled("PPPPP ll Pi Pi Pi ii f i Pi P Pi Pi Pi Pi Pz d P P"))
    assert len(_C.SYMBOLS["egc_gat_backward_dropout_f32"][1]) == 33
    restype, args = _C.SYMBOLS["egc_collate"]
    assert restype is C.c_int and args[3:] == spelled("Pl PPP i ll Pz PP")
    for got, struct in zip(args[:3], (_C.EgcCollateStore, _C.EgcCollateFields, _C.EgcCollateOut)):
        assert issubclass(got, C._Pointer) and got._type_ is struct
    assert len({a._type_ for a in args[:3]}) == 3
    assert _C.SYMBOLS["egc_last_error"] == (C.c_char_p, []) and _C.SYMBOLS["egc_version"] == (C.c_char_p, [])
    assert _C.SYMBOLS["egc_coo_to_csr_workspace_bytes"] == (Z, [L, L])
    assert _C.SYMBOLS["egc_gather_plan_launches"] == (L, []) and _C.SYMBOLS["egc_gather_plan_form"] == (I, [L, L, I])
    assert len(_C.SYMBOLS) == 128 and len(_C.ABI.structs) == 9 and len(_C.ABI.constants) == 78
    assert (_C.WEIGHT_GRAD_TILE_ROWS, _C.WEIGHT_GRAD_TILE_COLS, _C.WEIGHT_GRAD_MAX_SUM_COLS) == (128, 192, 128)


def test_struct_layouts_spelled_by_hand():
    g = _C.EgcGraph
    assert g is _C.ABI.structs["egc_graph"] and g.__name__ == "EgcGraph"
    assert C.sizeof(g) == 13 * 8 + 2 * 8 + 2 * 4 and g.n_chunks.offset == 72 and g.gather_plan_form_looped.offset == 124
    assert dict(g._fields_)["rowptr"] is P and dict(g._fields_)["n_src_rows"] is L and dict(g._fields_)["gather_plan_form_raw"] is I
    h = _C.EgcHead
    assert C.sizeof(h) == 4 + 5 * 4 + 7 * 32 + 2 * 32 + 8 * 32 and h.weight.offset == 24 and h.eps.offset == 248 and h.z.offset == 312
    assert dict(h._fields_)["sizes"] is I * 5 and dict(h._fields_)["eps"] is D * 4 and dict(h._fields_)["d_bias"] is P * 4
    f = _C.EgcCollateFields
    assert C.sizeof(_C.EgcCollateField) == 32 and _C.EgcCollateField.fill_bits.offset == 24
    assert C.sizeof(f) == 8 + 2 * 8 * 32 and f.n_graph.offset == 4 and f.node.offset == 8 and f.graph.offset == 8 + 8 * 32
    assert dict(f._fields_)["graph"] is _C.EgcCollateField * 8
    assert [n for n, _ in _C.EgcTypedRel._fields_][:4] == ["rowptr", "col", "pre_rowptr", "in_"] and _C.EgcTypedRel.in_.offset == 24
    assert C.sizeof(_C.EgcLayer) == 19 * 4 and C.sizeof(_C.EgcPost) == 32


def test_constants_spelled_by_hand():
    assert (_C.AGGR_SYMNORM, _C.ENCODER_MAX_TABLE_ROWS, _C.GP_HEADER_INTS, _C.PNA_INVERSE_LINEAR, _C.COLLATE_MAX_GRAPHS,
            _C.TOKEN_HEAD_MAX_IN, _C.MAX_WEIGHT_WIDTH) == (6, 1 << 20, 16, 4, 4096, 384, 2048)
    assert (_C.OK, _C.ERR_INVALID, _C.ERR_WORKSPACE, _C.ERR_HIP, _C.ERR_UNSUPPORTED) == (0, 1, 2, 3, 4)
    assert _C._STATUS == {1: "EGC_ERR_INVALID", 2: "EGC_ERR_WORKSPACE", 3: "EGC_ERR_HIP", 4: "EGC_ERR_UNSUPPORTED"}
    assert _C.EGC_MAX_AGGRS == _C.MAX_AGGRS == 8


SNIPPET = """
/* a comment with int egc_not_declared(void); inside */
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* egc_stream_t;  // a handle
typedef enum { EGC_A, EGC_B, EGC_C = 7, EGC_D } egc_e;
#define EGC_N (1 << 3)
#define EGC_M (EGC_N + EGC_D)
typedef struct egc_item { const float* p; int32_t a, b; double w[EGC_N]; int64_t* q[2]; int class; } egc_item;
typedef struct { egc_item one; egc_item many[EGC_M - 14]; const float* const* pp; egc_stream_t s; } egc_box;
int egc_f(const egc_item* item, egc_box* box, const egc_item* const* items, const float* const* rows, int32_t ids[], egc_stream_t s);
const char* egc_g(void);
size_t egc_h();
#ifdef __cplusplus
}
#endif
#endif /* X_H */
"""


def test_every_construct_on_a_snippet():
    abi = _abi.read_header(SNIPPET)
    assert abi.constants == {"EGC_A": 0, "EGC_B": 1, "EGC_C": 7, "EGC_D": 8, "EGC_N": 8, "EGC_M": 16}
    assert abi.enums == {"egc_e": {"EGC_A": 0, "EGC_B": 1, "EGC_C": 7, "EGC_D": 8}}
    item, box = abi.structs["egc_item"], abi.structs["egc_box"]
    assert item._fields_ == [("p", P), ("a", I), ("b", I), ("w", D * 8), ("q", P * 2), ("class_", C.c_int)]
    assert box._fields_ == [("one", item), ("many", item * 2), ("pp", P), ("s", P)]
    restype, args = abi.prototypes["egc_f"]
    assert restype is C.c_int and args[0]._type_ is item and args[1]._type_ is box and args[2:] == [P, P, P, P]
    assert abi.prototypes["egc_g"] == (C.c_char_p, []) and abi.prototypes["egc_h"] == (Z, [])
    assert list(abi.prototypes) == ["egc_f", "egc_g", "egc_h"]


@pytest.mark.parametrize("text,named", [
    ("int egc_f(int32_t a, unsigned b);", "unsigned"),                                   # an unknown type
    ("long egc_f(void);", "long"),
    ("int egc_f(void);\nstatic\ntypedef void* egc_stream_t;", "static"),                  # a stray token between declarations
    ("int egc_f(void); ;", ";"),
    ("#define EGC_X 1.5", "1.5"),                                                        # a non-integer #define EGC_...
    ("#define EGC_X \"text\"", "text"),
    ("#define EGC_X(a) (a)", "(a) (a)"),
    ("#define EGC_X EGC_UNKNOWN", "EGC_UNKNOWN"),
    ("#define OTHER 1", "#define OTHER 1"),
    ("typedef struct { egc_missing m; } egc_s;", "egc_missing"),                          # a member of an undeclared struct type
    ("typedef struct { int32_t a[EGC_NONE]; } egc_s;", "EGC_NONE"),
    ("typedef struct { int32_t a } egc_s;", "int32_t a"),
    ("typedef enum { EGC_A = 1, other } egc_e;", "other"),
    ("typedef struct { void v; } egc_s;", "void"),
    ("#if 0\nint egc_f(void);\n#endif", "#if 0"),
])
def test_what_the_reader_does_not_understand_raises_and_names_the_text(text, named):
    with pytest.raises(_abi.AbiError) as err:
        _abi.read_header(text)
    assert named in str(err.value)


def test_a_missing_header_says_so(monkeypatch):
    monkeypatch.setattr(_C, "_HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(RuntimeError, match="no_such_header.h is missing"):
        _C._read_abi()


SWITCH_CASES = {"EGC_T_UNSET": None, "EGC_T_EMPTY": "", "EGC_T_ZERO": "0", "EGC_T_ONE": "1", "EGC_T_ZEROS": "00", "EGC_T_NO": "no"}
SWITCH_WANT = {"EGC_T_UNSET": False, "EGC_T_EMPTY": False, "EGC_T_ZERO": False, "EGC_T_ONE": True, "EGC_T_ZEROS": True, "EGC_T_NO": True}


def test_on_off_switches_read_alike_in_cpp_and_python(monkeypatch):
    subprocess.run(["bash", os.path.join(ROOT, "tests", "env_on", "build.sh")], check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if k not in SWITCH_CASES}
    env.update({k: v for k, v in SWITCH_CASES.items() if v is not None})
    r = subprocess.run([os.path.join(ROOT, "tests", "env_on", "_build", "env_on_check"), *SWITCH_CASES], env=env, capture_output=True,
                       text=True, check=True, timeout=60)
    assert dict(line.split() for line in r.stdout.splitlines()) == {k: "on" if v else "off" for k, v in SWITCH_WANT.items()}
    for name, value in SWITCH_CASES.items():
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
        assert _C.env_flag(name) is SWITCH_WANT[name], name
