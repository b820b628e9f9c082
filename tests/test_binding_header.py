"""The ctypes binding is derived from the text of include/piccolo_hip.h (piccolo_amd/_header.py).  CPU checks: the parser's rules on small
header strings, the real header against an independent scan of its text, and struct layouts and constants against the C compiler."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import REPO
from piccolo_amd._header import Header, PiccoloHipError

HEADER = os.path.join(REPO, "include", "piccolo_hip.h")

SMALL = """
/* a block comment with pcl_foo( and a ) and a ; and
   #define PCL_NOT 1
   // inside */
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PCL_NEG (-2)   /* parenthesised, negative */
#define PCL_SEVEN 7 // trailing comment
#define PCL_EXPR ((int64_t)1 << 27)
// a line comment with pcl_bar(int x); and a )
typedef struct pcl_blk {
    double a, b;      /* two in one declaration */
    int32_t k;        // then padding
    const float *dev; /* a device address held on the host */
    int64_t w[4];
    double m[3];
} pcl_blk;
int pcl_abi_version(void);
const char *pcl_name(int code);
void pcl_free(void *handle);
void *pcl_make(int n);
int64_t pcl_broken(const float *xyz,
                   int64_t n,   /* pcl_no( */
                   double q, float f, size_t bytes);
int pcl_imgs(const float *const *imgs_host, const void *const *panos_host, int n);
int pcl_host_dev(const float *lo_host, const float *lo, int *count_host, int *count, const uint64_t *addr_host, const uint64_t *addr);
int pcl_blocks(const pcl_blk *blk_host, const pcl_blk *params, pcl_blk *out, const char *path);
size_t pcl_formats(int levels, const int *formats);
#ifdef __cplusplus
}
#endif
#endif
"""


@pytest.fixture(scope="module")
def small():
    return Header(SMALL, "small.h")


def test_prototypes_comments_and_line_breaks(small):
    vp = C.c_void_p
    assert sorted(small.signatures) == ["pcl_abi_version", "pcl_blocks", "pcl_broken", "pcl_formats", "pcl_free", "pcl_host_dev", "pcl_imgs",
                                        "pcl_make", "pcl_name"]                     # nothing from a comment
    assert small.signatures["pcl_abi_version"] == (C.c_int, [])                    # a void parameter list
    assert small.signatures["pcl_name"] == (C.c_char_p, [C.c_int])                 # const char * return
    assert small.signatures["pcl_free"] == (None, [vp])                            # void return
    assert small.signatures["pcl_make"] == (vp, [C.c_int])
    assert small.signatures["pcl_broken"] == (C.c_int64, [vp, C.c_int64, C.c_double, C.c_float, C.c_size_t])      # three lines, a comment inside


def test_pointer_rules(small):
    vp, P = C.c_void_p, C.POINTER
    assert small.signatures["pcl_imgs"][1] == [P(vp), P(vp), C.c_int]              # T *const *x_host: a host array of addresses
    assert small.signatures["pcl_host_dev"][1] == [P(C.c_float), vp, P(C.c_int), vp, P(C.c_uint64), vp]            # _host against device
    blk = small.structs["pcl_blk"]
    assert small.signatures["pcl_blocks"][1] == [P(blk), P(blk), vp, C.c_char_p]   # const struct *: a host block; struct *: a device record
    assert small.signatures["pcl_formats"] == (C.c_size_t, [C.c_int, P(C.c_int)])  # the named exception


def test_struct_fields_and_arrays(small):
    blk = small.structs["pcl_blk"]
    assert [name for name, _ in blk._fields_] == ["a", "b", "k", "dev", "w", "m"]
    assert [t for _, t in blk._fields_][:4] == [C.c_double, C.c_double, C.c_int32, C.c_void_p]
    assert blk.w.size == 32 and blk.m.size == 24 and blk._fields_[4][1]._length_ == 4 and blk._fields_[4][1]._type_ is C.c_int64
    assert (blk.a.offset, blk.b.offset, blk.k.offset, blk.dev.offset, blk.w.offset, blk.m.offset) == (0, 8, 16, 24, 32, 64)
    assert C.sizeof(blk) == 88


def test_defines(small):
    assert small.constants == {"PCL_NEG": -2, "PCL_SEVEN": 7}                      # not the guard, not the expression, not the comment's
    assert small.constant("PCL_NEG") == -2
    with pytest.raises(PiccoloHipError, match=r"small\.h.*PCL_EXPR"):
        small.constant("PCL_EXPR")


@pytest.mark.parametrize("decl", [
    "int pcl_x(long double v);",                   # an unknown scalar
    "int pcl_x(const pcl_nothing *p_host);",       # an unknown struct
    "int pcl_x(char *buf);",                       # only const char * is a string
    "int pcl_x(const float *const *imgs);",        # an array of addresses must be a host array
    "int pcl_x(const float **const *p_host);",
    "int pcl_x(int);",                             # no parameter name
    "unsigned pcl_x(int a);",                      # an unknown return type
    "typedef struct s { long double v; } s;",
    "int pcl_x(int a) { return a; }",              # not a prototype
])
def test_what_the_rules_do_not_know_raises(decl):
    with pytest.raises(PiccoloHipError, match=r"bad\.h"):
        Header("#define A 1\n" + decl + "\n", "bad.h")


def test_a_missing_header_names_the_file(tmp_path):
    with pytest.raises(PiccoloHipError, match="nowhere.h"):
        Header.read(str(tmp_path / "nowhere.h"))


# ---- the real header ----

def raw_declarations():
    """name -> parameter text of every prototype, by a scan that shares nothing with the parser but the comment stripping."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m[1]: m[2] for m in re.finditer(r"\b(pcl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}


def test_every_prototype_is_bound_with_its_argument_count():
    from piccolo_amd import _lib
    from test_abi import declared_symbols
    raw = raw_declarations()
    assert sorted(raw) == declared_symbols() == sorted(_lib.SIGNATURES)
    for name, params in raw.items():
        want = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(_lib.SIGNATURES[name][1]) == want, name


def test_the_two_documented_exceptions():
    from piccolo_amd import _lib
    P = C.POINTER
    assert _lib.SIGNATURES["pcl_pano_pyramid_bytes"][1][3] == P(C.c_int) and _lib.SIGNATURES["pcl_pano_pyramid"][1][4] == P(C.c_int)
    assert _lib.SIGNATURES["pcl_gd_step_from_grads"][1][5] == P(_lib.GdHyper)
    assert _lib.SIGNATURES["pcl_align_vote"][1][4:6] == [P(_lib.AlignParams), C.c_void_p]       # the out record lives on the device


CONSTANTS = ("ABI_VERSION", "RESULT_STRIDE", "GD_RESULT_STRIDE", "GD_SEQUENTIAL", "GD_BATCH", "PANO_F32", "PANO_U8", "PANO_F16", "PANO_U8P", "PANO_U8V",
             "ROBUST_TRUNC", "ROBUST_HUBER", "GD_MAX_ROOMS", "GD_PRUNE_MAX")
STRUCTS = {"pcl_gd_hyper": "GdHyper", "pcl_gn_hyper": "GnHyper", "pcl_gd_room": "GdRoom", "PclAlignParams": "AlignParams", "PclAlignOut": "AlignOut"}


def test_struct_layouts_and_constants_match_the_compiler(tmp_path):
    from piccolo_amd import _lib, build
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "piccolo_hip.h"', 'int main(void) {']
    for cname, pyname in STRUCTS.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (pyname, cname))
        for field, _ in getattr(_lib, pyname)._fields_:
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (pyname, field, cname, field, cname, field))
    for name in CONSTANTS:
        lines.append('    printf("%s %%lld\\n", (long long)PCL_%s);' % (name, name))
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([build.hipcc(), "-x", "c", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])          # host only
    said = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        key, *values = line.split()
        said[key] = tuple(int(v) for v in values)
    want = {name: (getattr(_lib, name),) for name in CONSTANTS}
    for pyname in STRUCTS.values():
        cls = getattr(_lib, pyname)
        want[pyname] = (C.sizeof(cls),)
        for field, _ in cls._fields_:
            want["%s.%s" % (pyname, field)] = (getattr(cls, field).offset, getattr(cls, field).size)
    assert said == want
    assert _lib.ALIGN_OUT_WORDS * 8 == said["AlignOut"][0] and len(_lib.GdHyper._fields_) == 12 and len(_lib.AlignOut._fields_) == 8
