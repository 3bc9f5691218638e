"""Test helper: the compiled reference's regex_search (oracle/_ref/libkrep_ref_avx2.so) called through ctypes with a regex_t that
libc's regcomp fills in a 256-byte buffer (glibc's regex_t is 64 bytes), and the libc probe of an atom's byte class.

TEST INFRASTRUCTURE: imported by the regex tests only."""
from __future__ import annotations

import contextlib
import ctypes as C
import locale
import os

import numpy as np

import oracle_lib as ol
from krep_amd import abi

REG_EXTENDED, REG_ICASE, REG_NEWLINE, REG_STARTEND = 1, 2, 4, 4  # glibc <regex.h>: cflags 1 / 2 / 4, eflags REG_STARTEND = 1 << 2

_libc = C.CDLL(None)
_libc.regcomp.restype = C.c_int
_libc.regcomp.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
_libc.regexec.restype = C.c_int
_libc.regexec.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_int]
_libc.regfree.restype = None
_libc.regfree.argtypes = [C.c_void_p]


class Regmatch(C.Structure):
    _fields_ = [("rm_so", C.c_int), ("rm_eo", C.c_int)]


class Compiled:
    """regcomp(pattern, REG_EXTENDED | REG_NEWLINE [| REG_ICASE]) — the flags of krep.c:2148"""

    def __init__(self, pattern: bytes, case_sensitive: bool = True):
        self.buf = C.create_string_buffer(256)
        rc = _libc.regcomp(self.buf, pattern, REG_EXTENDED | REG_NEWLINE | (0 if case_sensitive else REG_ICASE))
        if rc:
            raise ValueError(f"regcomp({pattern!r}) = {rc}")

    @property
    def ptr(self):
        return C.cast(self.buf, C.c_void_p)

    def matches_byte(self, b: int) -> bool:
        m = Regmatch(0, 1)
        t = C.create_string_buffer(bytes([b]), 2)
        return _libc.regexec(self.buf, t, 1, C.byref(m), REG_STARTEND) == 0 and m.rm_so == 0 and m.rm_eo == 1

    def __del__(self):
        try:
            _libc.regfree(self.buf)
        except Exception:
            pass


_class_cache = {}


def probe_class(atom: bytes, case_sensitive: bool = True) -> bytes:
    """The bytes libc's regexec matches with `atom` compiled alone: the class of the atom."""
    key = (atom, case_sensitive)
    if key not in _class_cache:
        c = Compiled(atom, case_sensitive)
        _class_cache[key] = bytes(b for b in range(256) if c.matches_byte(b))
    return _class_cache[key]


@contextlib.contextmanager
def c_locale():
    """LC_CTYPE = "C" for the duration: the locale the reference runs in (krep never calls setlocale(), Python does at start-up).
    In a multibyte locale libc's regexec matches characters instead of bytes and krep_gpu_regex_compile() takes no pattern."""
    old = locale.setlocale(locale.LC_CTYPE)
    locale.setlocale(locale.LC_CTYPE, "C")
    try:
        yield
    finally:
        locale.setlocale(locale.LC_CTYPE, old)


def available() -> bool:
    return ol.ref_available(abi.REF_AVX2)


_ref = {}


def _lib():
    if "l" not in _ref:
        L = C.CDLL(os.path.join(ol.REF_DIR, "libkrep_ref_avx2.so"))
        L.regex_search.restype = C.c_uint64
        L.regex_search.argtypes = [C.POINTER(abi.SearchParams), C.c_void_p, C.c_size_t, C.POINTER(abi.MatchResult)]
        L.match_result_init.restype = C.POINTER(abi.MatchResult)
        L.match_result_init.argtypes = [C.c_uint64]
        L.match_result_free.restype = None
        L.match_result_free.argtypes = [C.POINTER(abi.MatchResult)]
        _ref["l"] = L
    return _ref["l"]


def params(pattern: bytes, **kw) -> abi.Params:
    return abi.Params([pattern], regex=True, **kw)


def call(pattern: bytes, text, want_result=True, **kw):
    """regex_search of the compiled reference -> (returned count, positions[(n, 2) uint64] or None)"""
    L = _lib()
    p = params(pattern, **kw)
    comp = Compiled(pattern, p.s.case_sensitive)
    p.s.compiled_regex = comp.ptr
    tb = ol.TextBuf(text if isinstance(text, np.ndarray) else bytes(text))
    res = L.match_result_init(16) if want_result else None
    try:
        ret = L.regex_search(p.ref, tb.ptr, tb.n, res)
        pos = abi.result_positions(res) if res else None
    finally:
        if res:
            L.match_result_free(res)
    return int(ret), pos
