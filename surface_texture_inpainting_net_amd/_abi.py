"""The Python view of the C ABI, read from include/stin_hip.h: the header is the only place where a prototype, a struct
layout or an integer constant is written down.  The header's own style is the input format - one declaration per `;`,
`stin_` prefixed entry points, plain scalar types, named parameters, integer `#define STIN_*` - and anything else is an
error that names the header line, never a guess.
"""
import ctypes
import os
import re
import struct

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'stin_hip.h')


class StinLibraryError(RuntimeError):
    pass


# by-value C type -> (ctypes type, struct code); every pointer and `typedef void*` handle is _POINTER
_SCALARS = {'int': (ctypes.c_int, 'i'), 'int32_t': (ctypes.c_int, 'i'), 'uint32_t': (ctypes.c_uint32, 'I'),
            'int64_t': (ctypes.c_int64, 'q'), 'uint64_t': (ctypes.c_uint64, 'Q'), 'size_t': (ctypes.c_size_t, 'Q'),
            'float': (ctypes.c_float, 'f'), 'double': (ctypes.c_double, 'd')}
_POINTER = (ctypes.c_void_p, 'Q')
_SPACE = re.compile(r'\s*')
_INTEGER = r'(-?(?:0[xX][0-9a-fA-F]+|\d+))'
_DEFINE = re.compile(r'#define\s+(STIN_\w+)\s+(?:\(%s\)|%s)$' % (_INTEGER, _INTEGER))
_STRUCT = re.compile(r'typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;')
_TYPEDEF = re.compile(r'typedef\s+(\w+)\s*(\*|\s)\s*(\w+)\s*;')
_PROTOTYPE = re.compile(r'(const\s+char\s*\*|\w+)\s*(stin_\w+)\s*\(([^()]*)\)\s*;')
_FIELD = re.compile(r'\s*(?:const\s+)?(\w+)\b(.*)$', re.S)              # type, then comma separated declarators:
_DECLARATOR = re.compile(r'\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*$')      # `x`, `*x` or `x[3]`
_PARAMETER = re.compile(r'\s*(?:const\s+)?(\w+)\s*(\*|\s)\s*\w+\s*$')  # type, `*` or a space, a name; never a `[`


class Record:
    """One struct of the header, packed by FIELD NAME only: `fields` in declaration order, `format` / `size` of the packed
    little-endian layout.  pack(name=value, ...) -> bytes; a field that is not named is zero, an array field (`int64_t
    reserved[3]`) is one name that takes a sequence of its length.  Names were resolved to positions when the header was
    read: a call copies the row of zeros, assigns and packs."""
    __slots__ = ('name', 'fields', 'format', 'size', '_pack', '_zeros', '_at')

    def __init__(self, name, fields):
        """fields: [(field name, struct code, element count)]"""
        self.name, self.fields = name, tuple(f for f, _, _ in fields)
        packed = '<' + ''.join(code * n for _, code, n in fields)               # little-endian, no padding
        st = struct.Struct(packed)
        self.format, self.size, self._pack = st.format, st.size, st.pack
        self._at, at = {}, 0
        for f, _, n in fields:
            self._at[f] = at if n == 1 else slice(at, at + n)
            at += n
        self._zeros = [0] * at

    def pack(self, **values):
        row, at = self._zeros[:], self._at
        try:
            for f, v in values.items():
                row[at[f]] = v
            return self._pack(*row)
        except KeyError:
            raise StinLibraryError('%s has no field %r' % (self.name, f)) from None
        except (struct.error, TypeError) as e:      # a value of the wrong kind, or an array field given another length
            raise StinLibraryError('%s: cannot pack %s (%s)' % (self.name, ', '.join(sorted(values)), e)) from None


def _pieces(text, sep, start):
    """The `sep`-separated pieces of text[start:...] with the position of each one's first character."""
    for piece in text.split(sep):
        yield piece, start + len(piece) - len(piece.lstrip())
        start += len(piece) + 1


class _Header:
    def __init__(self, text, where):
        self.where, self.types = where, dict(_SCALARS)
        self.signatures, self.structs, self.constants = {}, {}, {}
        blank = lambda m: re.sub(r'[^\n]+', lambda s: ' ' * len(s.group(0)), m.group(0))     # positions keep their lines
        self.text = re.sub(r'/\*.*?\*/', blank, text, flags=re.S)
        self.text = re.sub(r'^(?:extern "C" \{|\})$', blank, self.text, flags=re.M)          # the C++ bracket's two lines
        self.directives()
        self.text = re.sub(r'^[ \t]*#.*$', blank, self.text, flags=re.M)
        self.declarations()

    def fail(self, pos, what):
        raise StinLibraryError('%s:%d: %s' % (self.where, self.text.count('\n', 0, pos) + 1, what))

    def kind(self, name, star, pos):
        """('float', '*') / ('stin_stream_t', '') / ('int', '') -> (ctypes type, struct code)"""
        if star:
            return _POINTER
        if self.types.get(name) is None:            # (None: an element type such as stin_bf16_t, only ever pointed to)
            self.fail(pos, 'unknown type %r' % name)
        return self.types[name]

    def directives(self):
        """Integer #defines; besides them only #include, the include guard and the __cplusplus bracket may appear."""
        guard = None
        for line in re.finditer(r'^[ \t]*#.*$', self.text, flags=re.M):
            words, define = line.group(0).split(), _DEFINE.match(line.group(0).strip())
            if define:
                self.constants[define.group(1)] = int(define.group(2) or define.group(3), 0)
            elif words[0] == '#ifndef' and guard is None and len(words) == 2:
                guard = words[1]
            elif words not in (['#define', guard], ['#ifdef', '__cplusplus'], ['#endif']) and words[0] != '#include':
                self.fail(line.start(), 'neither `#define STIN_<NAME> <integer literal>` nor an include / guard line')

    def declarations(self):
        pos = _SPACE.match(self.text).end()
        while pos < len(self.text):
            for pattern, read in ((_STRUCT, self.struct), (_TYPEDEF, self.typedef), (_PROTOTYPE, self.prototype)):
                m = pattern.match(self.text, pos)
                if m:
                    read(m)
                    break
            else:
                self.fail(pos, 'neither a typedef nor a stin_* prototype of the header style')
            pos = _SPACE.match(self.text, m.end()).end()

    def typedef(self, m):
        """A handle (`typedef void* x`: a pointer) or an element type (`typedef uint16_t x`: usable behind `*` only, unless
        the base is a known scalar)."""
        self.types[m.group(3)] = _POINTER if m.group(2) == '*' else self.types.get(m.group(1))

    def struct(self, m):
        *fields, tail = _pieces(m.group(1), ';', m.start(1))
        if tail[0].strip() or not fields:
            self.fail(tail[1], 'struct field without `;`')
        named = []
        for field, at in fields:
            f = _FIELD.match(field)
            for declarator in f.group(2).split(',') if f else ['']:
                d = _DECLARATOR.match(declarator)
                if d is None:
                    self.fail(at, 'cannot split the declarator %r' % ' '.join(field.split()))
                if any(d.group(2) == n for n, _, _ in named):
                    self.fail(at, 'second field %r' % d.group(2))
                named.append((d.group(2), self.kind(f.group(1), d.group(1), at)[1], int(d.group(3) or 1)))
        record = Record(m.group(2), named)          # (packed without padding: right only if the C layout has none either)
        codes = record.format[1:]
        if record.size != struct.calcsize('@%s0%s' % (codes, max(codes, key=struct.calcsize))):
            self.fail(m.start(2), '%s needs padding in C' % m.group(2))
        self.structs[m.group(2)] = record

    def prototype(self, m):
        ret, name, params = m.groups()
        if name in self.signatures:
            self.fail(m.start(2), 'second declaration of %s' % name)
        argtypes = []
        for param, at in _pieces(params, ',', m.start(3)) if params.strip() != 'void' else ():
            p = _PARAMETER.match(param)
            if p is None:
                self.fail(at, 'cannot split the parameter %r (type, optional `*`, name)' % ' '.join(param.split()))
            argtypes.append(self.kind(p.group(1), p.group(2) == '*', at)[0])
        restype = ctypes.c_char_p if '*' in ret else self.kind(ret, '', m.start(1))[0]
        self.signatures[name] = (restype, argtypes)


def parse_header(text, where='stin_hip.h'):
    """-> (SIGNATURES, STRUCTS, CONSTANTS) of a header written in the style of include/stin_hip.h."""
    h = _Header(text, where)
    return h.signatures, h.structs, h.constants


def read_header(path=HEADER_PATH):
    try:
        with open(path) as f:
            return parse_header(f.read(), path)
    except OSError as e:
        raise StinLibraryError('cannot read the C ABI header %s: %s' % (path, e))
