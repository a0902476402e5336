"""The PLY contract of scene_io.read_ply, restated on its own: a header parser, a body decode with numpy structured dtypes (binary)
or line by line (ascii), the fan triangulation as a loop over the records (a file of triangles only is its own result and
skips the loop), and the reference's per-face label vote
(preprocessing/graph_level_generation.py:328-336) as its numpy loop.  It shares no code with the package; tests/test_ply.py holds
it to files whose bytes are written out in the test with struct.pack and whose values are known by construction.

The contract.  Header: `ply`, one `format` line, `comment` / `obj_info` lines, `element <name> <count>` each followed by its
`property <type> <name>` / `property list <count type> <type> <name>` lines, `end_header`; the body starts at the next byte.  Types:
char uchar short ushort int uint float double or int8 .. float64.  Body: the elements in header order, each `count` records of its
properties in order; a list is its count followed by that many entries.  Ascii: one record per line, numbers read as python
float / int and stored in the property's type.  Result (numpy, the keys of read_ply):
    vertices float64 [N, 3]; faces int64 [F, 3], a polygon (v0 .. vk-1) as the fan (v0, v1, v2), (v0, v2, v3), ... in record order;
    colors float64 = uint8 / 255.0 and colors_u8, when red green blue are uchar; normals float64, when nx ny nz exist;
    vertex_properties / face_properties: every other scalar property, int64 or float64, one entry per record.
Errors: ValueError for a body that ends early or a polygon of fewer than 3 vertices (and, with triangulate=False, of more);
IndexError naming the first face with an index outside [0, N).
"""
import re
import struct

import numpy as np

CANON = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
         'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}
STRUCT_CODE = {'i1': 'b', 'u1': 'B', 'i2': 'h', 'u2': 'H', 'i4': 'i', 'u4': 'I', 'f4': 'f', 'f8': 'd'}
LONG_NAME = {'i1': 'int8', 'u1': 'uint8', 'i2': 'int16', 'u2': 'uint16', 'i4': 'int32', 'u4': 'uint32', 'f4': 'float32', 'f8': 'float64'}
_LINE = re.compile(rb'([^\n]*)\n')


def parse_header(blob):
    """bytes -> (format, [(element, count, [(property, numpy code, count code or None)])], body offset)"""
    fmt, elements, at, n = None, [], 0, 0
    while True:
        m = _LINE.match(blob, at)
        if m is None:
            raise ValueError('no end_header')
        at, n = m.end(), n + 1
        line = m.group(1).decode('latin-1').strip()
        w = line.split()
        if n == 1:
            if line != 'ply':
                raise ValueError('line 1: %r' % line)
        elif not w or w[0] in ('comment', 'obj_info'):
            pass
        elif w[0] == 'end_header':
            break
        elif w[0] == 'format' and len(w) == 3 and fmt is None and w[1] in ('ascii', 'binary_little_endian', 'binary_big_endian'):
            fmt = w[1]
        elif w[0] == 'element' and len(w) == 3 and w[2].isdigit() and w[1] not in [e[0] for e in elements]:
            elements.append((w[1], int(w[2]), []))
        elif w[0] == 'property' and elements and len(w) == 3 and w[1] in CANON and w[2] not in [p[0] for p in elements[-1][2]]:
            elements[-1][2].append((w[2], CANON[w[1]], None))
        elif (w[0] == 'property' and elements and len(w) == 5 and w[1] == 'list' and w[2] in CANON and w[3] in CANON
              and CANON[w[2]][0] != 'f' and w[4] not in [p[0] for p in elements[-1][2]]):
            elements[-1][2].append((w[4], CANON[w[3]], CANON[w[2]]))
        else:
            raise ValueError('line %d: %r' % (n, line))
    if fmt is None:
        raise ValueError('no format line')
    return fmt, elements, at


def header_like_the_package(blob):
    """parse_header in the shape of scene_io.read_ply_header (without comments and obj_info)."""
    fmt, elements, at = parse_header(blob)
    return {'format': fmt, 'body_offset': at,
            'elements': [{'name': e, 'count': c, 'properties': [{'name': p, 'type': LONG_NAME[t], 'count_type': LONG_NAME.get(ct)}
                                                                  for p, t, ct in props]} for e, c, props in elements]}


def _number(token, code):
    if code[0] == 'f':
        return np.dtype(code).type(float(token))
    v = int(token)
    info = np.iinfo(code)
    if not info.min <= v <= info.max:
        raise ValueError('%r does not fit %s' % (token, code))
    return np.dtype(code).type(v)


def _records(blob, fmt, elements, at):
    """-> {element: ({scalar property: [values]}, [index lists] or None)} for vertex and face"""
    out = {}
    order = '>' if fmt == 'binary_big_endian' else '<'
    lines = blob[at:].decode('latin-1').split('\n') if fmt == 'ascii' else None
    lines = [l for l in lines if l.strip()] if lines is not None else None
    row = 0
    for name, count, props in elements:
        has_list = any(ct is not None for _, _, ct in props)
        if has_list and name != 'face':
            raise ValueError('element %r has a list property' % name)
        if sum(ct is not None for _, _, ct in props) > 1:
            raise ValueError('two lists')
        cols = {p: [] for p, _, ct in props if ct is None}
        polys = [] if has_list else None
        if fmt == 'ascii':
            if row + count > len(lines):
                raise ValueError('truncated: element %r' % name)
            for line in lines[row:row + count]:
                tok = line.split()
                i = 0
                for p, t, ct in props:
                    if i >= len(tok):
                        raise ValueError('truncated: a short line in element %r' % name)
                    if ct is None:
                        cols[p].append(_number(tok[i], t))
                        i += 1
                    else:
                        k = int(_number(tok[i], ct))
                        if k < 0 or i + 1 + k > len(tok):
                            raise ValueError('truncated: a short line in element %r' % name)
                        polys.append([int(_number(x, t)) for x in tok[i + 1:i + 1 + k]])
                        i += 1 + k
            row += count
        elif not has_list:
            dt = np.dtype([(p, order + t) for p, t, _ in props])
            if at + count * dt.itemsize > len(blob):
                raise ValueError('truncated: element %r' % name)
            block = np.frombuffer(blob, dtype=dt, count=count, offset=at)
            for p, t, _ in props:
                cols[p] = block[p].astype(t)
            at += count * dt.itemsize
        else:
            uniform = _uniform_lists(blob, order, props, count, at)
            if uniform is not None:
                block, at = uniform
                for p, t, ct in props:
                    if ct is None:
                        cols[p] = block[p].astype(t)
                    else:
                        polys = block[p]['ids'].astype(np.int64)
                out[name] = (cols, polys, {p: t for p, t, _ in props}, count)
                continue
            for _ in range(count):
                for p, t, ct in props:
                    try:
                        if ct is None:
                            cols[p].append(np.dtype(t).type(struct.unpack_from(order + STRUCT_CODE[t], blob, at)[0]))
                            at += np.dtype(t).itemsize
                        else:
                            k = struct.unpack_from(order + STRUCT_CODE[ct], blob, at)[0]
                            at += np.dtype(ct).itemsize
                            polys.append([int(v) for v in struct.unpack_from('%s%d%s' % (order, max(k, 0), STRUCT_CODE[t]), blob, at)])
                            at += max(k, 0) * np.dtype(t).itemsize
                    except struct.error:
                        raise ValueError('truncated: element %r' % name) from None
        if name in ('vertex', 'face'):
            out[name] = (cols, polys, {p: t for p, t, _ in props}, count)
    return out


def _uniform_lists(blob, order, props, count, at):
    """The records of a list element as ONE structured array when every list is as long as the first, else None."""
    head = 0
    for p, t, ct in props:
        if ct is not None:
            break
        head += np.dtype(t).itemsize
    if count == 0 or at + head + np.dtype(ct).itemsize > len(blob):
        return None
    k = struct.unpack_from(order + STRUCT_CODE[ct], blob, at + head)[0]
    if not 0 <= k <= 255:
        return None
    dt = np.dtype([(p, order + t) if c is None else (p, [('n', order + c), ('ids', order + t, (k,))]) for p, t, c in props])
    if at + count * dt.itemsize > len(blob):
        return None
    block = np.frombuffer(blob, dtype=dt, count=count, offset=at)
    if not bool((block[[p for p, _, c in props if c is not None][0]]['n'] == k).all()):
        return None
    return block, at + count * dt.itemsize


def _wide(values, code, count):
    a = np.asarray(values, dtype=code).reshape(count)
    return a.astype(np.float64) if code[0] == 'f' else a.astype(np.int64)


def decode(blob, triangulate=True):
    """The bytes of a PLY file -> the dict of read_ply as numpy arrays (without 'header')."""
    blob = bytes(blob)
    fmt, elements, at = parse_header(blob)
    rec = _records(blob, fmt, elements, at)
    vcols, _, vtypes, n = rec.get('vertex', ({}, None, {}, 0))
    fcols, polys, ftypes, nrec = rec.get('face', ({}, None, {}, 0))
    if n > 0 and not all(k in vcols for k in 'xyz'):
        raise ValueError('no x, y or z')
    mesh, used = {}, set()
    triple = lambda names, code: np.stack([np.asarray(vcols[k], dtype=vtypes[k]).reshape(n).astype(code) for k in names], axis=1)
    if all(k in vcols for k in 'xyz'):
        mesh['vertices'] = triple('xyz', np.float64)
        used |= set('xyz')
    else:
        mesh['vertices'] = np.zeros((0, 3), dtype=np.float64)
    tris = []
    if isinstance(polys, np.ndarray) and polys.shape[1] == 3:                # triangles are their own fans
        wrong = ((polys < 0) | (polys >= n)).any(axis=1)
        if wrong.any():
            raise IndexError('face %d has a vertex index outside [0, %d)' % (int(np.argmax(wrong)), n))
        tris, polys = polys, None
    for r, poly in enumerate([] if polys is None else polys.tolist() if isinstance(polys, np.ndarray) else polys):
        if len(poly) < 3 or (not triangulate and len(poly) != 3):
            raise ValueError('face %d has %d vertices' % (r, len(poly)))
        for t in range(len(poly) - 2):
            tri = (poly[0], poly[t + 1], poly[t + 2])
            if min(tri) < 0 or max(tri) >= n:
                raise IndexError('face %d has a vertex index outside [0, %d)' % (r, n))
            tris.append(tri)
    mesh['faces'] = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if all(vtypes.get(k) == 'u1' for k in ('red', 'green', 'blue')):
        mesh['colors_u8'] = triple(('red', 'green', 'blue'), np.uint8)
        mesh['colors'] = mesh['colors_u8'].astype(np.float64) / 255.0
        used |= {'red', 'green', 'blue'}
    if all(k in vcols for k in ('nx', 'ny', 'nz')):
        mesh['normals'] = triple(('nx', 'ny', 'nz'), np.float64)
        used |= {'nx', 'ny', 'nz'}
    mesh['vertex_properties'] = {k: _wide(v, vtypes[k], n) for k, v in vcols.items() if k not in used}
    mesh['face_properties'] = {k: _wide(v, ftypes[k], nrec) for k, v in fcols.items()}
    return mesh


def vote(faces, face_labels, num_vertices, num_classes):
    """The reference's loop (graph_level_generation.py:328-336) with its 22 as num_classes; a label outside [0, num_classes) is
    not counted -> (vertex labels int64 [N], True when such a label was met)."""
    hist = np.zeros((num_vertices, num_classes), dtype=np.int64)
    flagged = False
    for row_id in range(faces.shape[0]):
        if not 0 <= face_labels[row_id] < num_classes:
            flagged = True
            continue
        for i in range(3):
            hist[faces[row_id][i], face_labels[row_id]] += 1
    return np.argmax(hist, axis=1).astype(np.int64).reshape(num_vertices), flagged


# ------------------------------------------------------------------------------------------------------------------ test files
def make_ply(fmt, vertex_props, vertex_cols, face_props=(), face_cols=None, n_faces=None, comment=None, other=()):
    """The bytes of a PLY file, every number through struct.pack (binary) or repr (ascii).
    fmt: 'ascii' | 'binary_little_endian' | 'binary_big_endian'; vertex_props: [(type as written, name)]; vertex_cols: {name: values};
    face_props: [(type, name)] or [('list', count type, index type, name)]; face_cols: {name: values}, a list property's value is a
    list of index lists; comment: an extra comment line (its length shifts the body); other: [(element name, [(type, name)],
    {name: values})] written AFTER the faces."""
    n = len(next(iter(vertex_cols.values()))) if vertex_cols else 0
    face_cols = face_cols or {}
    if n_faces is None:
        n_faces = len(next(iter(face_cols.values()))) if face_cols else 0
    head = ['ply', 'format %s 1.0' % fmt]
    if comment is not None:
        head.append('comment ' + comment)
    groups = [('vertex', n, list(vertex_props), vertex_cols)]
    if face_props:
        groups.append(('face', n_faces, list(face_props), face_cols))
    for name, props, cols in other:
        groups.append((name, len(next(iter(cols.values()))), list(props), cols))
    for name, count, props, _ in groups:
        head.append('element %s %d' % (name, count))
        head += ['property ' + ' '.join(p) for p in props]
    head.append('end_header')
    out = [('\n'.join(head) + '\n').encode('ascii')]
    order = '>' if fmt == 'binary_big_endian' else '<'

    def put(value, type_name):
        code = CANON[type_name]
        if fmt == 'ascii':
            return repr(float(value)) if code[0] == 'f' else str(int(value))
        return struct.pack(order + STRUCT_CODE[code], value)

    for name, count, props, cols in groups:
        for r in range(count):
            parts = []
            for p in props:
                if p[0] == 'list':
                    ids = cols[p[3]][r]
                    parts.append(put(len(ids), p[1]))
                    parts += [put(v, p[2]) for v in ids]
                else:
                    parts.append(put(cols[p[1]][r], p[0]))
            out.append((' '.join(parts) + '\n').encode('ascii') if fmt == 'ascii' else b''.join(parts))
    return b''.join(out)


def same_mesh(got, want):
    """got: read_ply's dict (tensors), want: decode's (numpy): same keys, dtypes, shapes and bytes."""
    keys = set(got) - {'header'}
    assert keys == set(want), (sorted(keys), sorted(want))
    for k in sorted(keys):
        if isinstance(want[k], dict):
            assert set(got[k]) == set(want[k]), (k, sorted(got[k]), sorted(want[k]))
            pairs = [(k + '.' + n, got[k][n], want[k][n]) for n in want[k]]
        else:
            pairs = [(k, got[k], want[k])]
        for name, g, w in pairs:
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
            assert g.tobytes() == np.ascontiguousarray(w).tobytes(), name
