"""include/te_hip.h as ctypes prototypes: header text -> {name: (restype, [argtypes])}.  No library is loaded and no torch is
imported here.  The type vocabulary is closed; a prototype outside it raises instead of being guessed."""
import ctypes as C
import re

_SCALAR = {'int': C.c_int, 'int64_t': C.c_int64, 'float': C.c_float, 'double': C.c_double, 'te_stream_t': C.c_void_p}
_PROTO = re.compile(r'\s*([\w\s*]+?)\b(te_\w+)\s*\(([^()]*)\)\s*')


def strip(text):
    """the header without comments and preprocessor lines"""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    return re.sub(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', '', text, flags=re.M)


def abi_version(text):
    m = re.search(r'^[ \t]*#[ \t]*define[ \t]+TE_ABI_VERSION[ \t]+(\d+)', text, flags=re.M)
    if not m:
        raise RuntimeError('te_hip.h does not define TE_ABI_VERSION')
    return int(m.group(1))


def _words(decl):
    return [w for w in re.findall(r'\w+', decl) if w != 'const']


def _param(p, proto):
    if '*' in p or '[' in p:
        return C.c_void_p
    w = _words(p)                                   # type, then an optional name
    if not 1 <= len(w) <= 2 or w[0] not in _SCALAR:
        raise RuntimeError(f'te_hip.h: cannot bind parameter "{p.strip()}" of {proto}')
    return _SCALAR[w[0]]


def _result(r, proto):
    w = _words(r)
    if w == ['char'] and r.count('*') == 1:
        return C.c_char_p
    if '*' in r or len(w) != 1 or w[0] not in _SCALAR:
        raise RuntimeError(f'te_hip.h: cannot bind the return type "{r.strip()}" of {proto}')
    return _SCALAR[w[0]]


def parse(text):
    """every `ret te_name(params);` of the header, in header order"""
    out = {}
    for stmt in re.split(r'[;{}]', strip(text)):
        if not re.search(r'\bte_\w+\s*\(', stmt):
            continue
        m = _PROTO.fullmatch(stmt)
        if not m:
            raise RuntimeError(f'te_hip.h: cannot read the prototype "{" ".join(stmt.split())}"')
        ret, name, params = m.groups()
        proto = f'{name}({" ".join(params.split())})'
        params = [] if params.strip() in ('', 'void') else params.split(',')
        out[name] = (_result(ret, proto), [_param(p, proto) for p in params])
    return out
