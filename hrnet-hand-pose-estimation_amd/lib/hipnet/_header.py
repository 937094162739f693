"""Reader of include/hrnet_hip.h: the prototypes, structs and constants of the C ABI as ctypes, so that the binding
(hipnet._capi) states none of them a second time. Pure Python: no library, no torch, no GPU.

It reads the C that the header uses and nothing more. A declaration it does not fully understand raises ValueError with
that declaration's text: nothing is skipped and nothing defaults to int.

Two markers of the header carry what C's own types do not say:
  HR_HOST     on a pointer parameter: host memory the call reads or writes before it returns -> POINTER(element);
              an unmarked pointer is a device pointer or an address -> c_void_p
  hr_value_t  as a return type: a count, flag or mode. A function returns a status iff it is declared plain `int`.
"""
import collections
import ctypes
import re

Proto = collections.namedtuple('Proto', 'name restype status params text')   # params: [(name, ctypes type)]
Header = collections.namedtuple('Header', 'protos structs values')           # name -> Proto / Structure class / int

# spelling -> (element type or None for void, pointer depth); typedefs and structs of a header join its own copy
_BASE = {'void': (None, 0), 'char': (ctypes.c_char, 0), 'unsigned char': (ctypes.c_ubyte, 0),
         'int': (ctypes.c_int, 0), 'float': (ctypes.c_float, 0), 'double': (ctypes.c_double, 0),
         'long long': (ctypes.c_int64, 0), 'int64_t': (ctypes.c_int64, 0), 'int32_t': (ctypes.c_int32, 0)}
_INT = r'[-+]?(?:0[xX][0-9a-fA-F]+|\d+)'


def _declarator(text, types, decl, base=None):
    """'const float* const* srcs' -> (name, element, pointer depth, array extent or None, HR_HOST marked); `base`: the
    type a further declarator of one struct field shares with the first ('a, b' of 'int32_t a, b')"""
    m = re.fullmatch(r'([\w\s*]*?)(\w+)\s*(?:\[\s*(\d+)\s*\])?', text.strip())
    words = re.sub(r'\bconst\b', ' ', m.group(1).replace('*', ' ')).split() if m else None
    spelling = ' '.join(w for w in words or () if w != 'HR_HOST')
    if m is None or (spelling not in types if base is None else spelling):
        raise ValueError('hrnet_hip.h: cannot read {!r} in: {}'.format(text.strip(), decl))
    host = 'HR_HOST' in words
    base = base or types[spelling]
    return m.group(2), base[0], base[1] + m.group(1).count('*'), m.group(3) and int(m.group(3)), host


def _ctype(elem, depth, host, what, decl):
    if depth == 0 and elem is not None and not host:
        return elem
    if depth == 1 and elem is ctypes.c_char:
        return ctypes.c_char_p
    if depth == 1 and host and elem is not None:
        return ctypes.POINTER(elem)
    if depth == 1 and not host:
        return ctypes.c_void_p
    if depth == 2:
        return ctypes.POINTER(ctypes.c_void_p)
    raise ValueError('hrnet_hip.h: no ctypes type for {!r} in: {}'.format(what.strip(), decl))


def _struct(name, body, types, decl):
    fields = []
    for field in filter(None, (f.strip() for f in body.split(';'))):
        base = None
        for piece in field.split(','):
            fname, elem, depth, extent, host = _declarator(piece, types, decl, base)
            base = base or (elem, depth - piece.count('*'))
            # an unmarked pointer field is an address, whatever it points to
            ctype = ctypes.c_void_p if depth == 1 and not host else _ctype(elem, depth, host, piece, decl)
            fields.append((fname, ctype * extent if extent else ctype))
    return type(name, (ctypes.Structure,), {'_fields_': fields})


def _enum(body, values, decl):
    nxt = 0
    for item in filter(None, (t.strip() for t in body.split(','))):
        m = re.fullmatch(r'(\w+)(?:\s*=\s*({}|\w+))?'.format(_INT), item)
        if not m or m.group(1) in values or (m.group(2) and not re.fullmatch(_INT, m.group(2))
                                             and m.group(2) not in values):
            raise ValueError('hrnet_hip.h: cannot read enumerator {!r} in: {}'.format(item, decl))
        if m.group(2):
            nxt = values[m.group(2)] if m.group(2) in values else int(m.group(2), 0)
        values[m.group(1)] = nxt
        nxt += 1


def _proto(m, types, decl):
    if re.search(r'[()\[\]:]', m.group(3)):
        raise ValueError('hrnet_hip.h: cannot read the parameters of: ' + decl)
    _, elem, depth, _, host = _declarator(m.group(1) + ' _', types, decl)
    params = []
    for text in ([] if m.group(3).strip() == 'void' else m.group(3).split(',')):
        name, pelem, pdepth, _, phost = _declarator(text, types, decl)
        params.append((name, _ctype(pelem, pdepth, phost, text, decl)))
    return Proto(m.group(2), _ctype(elem, depth, host, m.group(1), decl),
                 re.sub(r'\bconst\b', '', m.group(1)).strip() == 'int', params, decl)


def parse(text):
    """header text -> Header(protos, structs, values)"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#[ \t]*ifdef __cplusplus\b.*?^[ \t]*#[ \t]*endif\b', '', text, flags=re.S | re.M)
    protos, structs, values, types = {}, {}, {}, dict(_BASE)
    for line in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(HR_\w+.*)$', text, flags=re.M):
        m = re.fullmatch(r'(\w+)(?:\s+({}))?\s*'.format(_INT), line)
        if not m:
            raise ValueError('hrnet_hip.h: cannot read: #define ' + line)
        if m.group(2):
            values[m.group(1)] = int(m.group(2), 0)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M).strip()
    # a declaration ends at a ';' outside braces; the declarations and the space between them are the whole text
    found = re.compile(r'\s*((?:[^;{}]|\{[^{}]*\})+);\s*')
    pos, decls = 0, []
    while pos < len(text):
        m = found.match(text, pos)
        if not m:
            raise ValueError('hrnet_hip.h: cannot read: ' + ' '.join(text[pos:].split())[:200])
        decls.append(' '.join(m.group(1).split()))
        pos = m.end()
    for decl in decls:
        m = re.fullmatch(r'typedef struct (\w+) \{(.*)\} (\w+)', decl)
        if m and m.group(1) == m.group(3):
            structs[m.group(1)] = _struct(m.group(1), m.group(2), types, decl)
            types[m.group(1)] = (structs[m.group(1)], 0)
            continue
        m = re.fullmatch(r'enum \{(.*)\}', decl)
        if m:
            _enum(m.group(1), values, decl)
            continue
        m = re.fullmatch(r'typedef ([\w\s*]+)', decl)
        if m:
            name, elem, depth, extent, host = _declarator(m.group(1), types, decl)
            if extent or host:
                raise ValueError('hrnet_hip.h: cannot read: ' + decl)
            types[name] = (elem, depth)
            continue
        m = re.fullmatch(r'([\w\s*]+?)\b(hrnet_\w+) ?\((.*)\)', decl)
        if not m or m.group(2) in protos:
            raise ValueError('hrnet_hip.h: cannot read: ' + decl)
        protos[m.group(2)] = _proto(m, types, decl)
    return Header(protos, structs, values)


def load(path):
    with open(path) as f:
        return parse(f.read())
