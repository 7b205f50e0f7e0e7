"""include/wmz.h (and the development probes' csrc/wmz_debug.h) as the C-ABI tests read them: by scans of their own, deliberately NOT
through world_modelz_amd._lib.parse_header -- the tests hold that reader, and the built library, against the headers."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wmz.h')
DEBUG_HEADER = os.path.join(ROOT, 'world_modelz_amd', 'csrc', 'wmz_debug.h')


def text(path=HEADER):
    with open(path) as f:
        return f.read()


def code(path=HEADER):
    """The header without its comments."""
    return re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text(path), flags=re.S)


def declared(path=HEADER):
    """Every wmz_name( of the header, the ones its comments speak of included: each has to be an entry point."""
    return set(re.findall(r'\b(wmz_[a-z0-9_]+)\s*\(', text(path)))


def arguments(name, path=HEADER):
    """The argument list of name's declaration, as written (comments stripped)."""
    found = re.findall(r'\b' + name + r'\s*\(([^()]*)\)\s*;', code(path))
    assert len(found) == 1, (name, found)
    return found[0]


def constants(prefix, path=HEADER):
    """{name: value} of the header's enumerators / #defines that start with prefix, in the order they are written."""
    return {n: int(v) for n, v in re.findall(r'\b(' + prefix + r'\w*)\s*=?\s*(\d+)\b', code(path))}


def assert_bound(lib, *names):
    """Each name is declared in include/wmz.h, has a ctypes signature and is exported by the built library."""
    from world_modelz_amd import _lib
    for n in names:
        assert n in declared(), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
