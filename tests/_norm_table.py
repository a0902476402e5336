"""The routes of the norm kernels as a hand-written table: one point per route, threshold and refusal of stin_colreduce_* (asked
of the host-only query stin_colreduce_route) and of the channels-per-lane classes of the elementwise passes
(stin_norm_lane_class).  Shared by tests/test_norm_geometry.py (CPU: every point reaches what its line names, at 256 and at 64
compute units) and tests/test_norm_exact_gpu.py (GPU: the shapes it runs are chosen and checked through the same query with the
device's CU count).  The numbers are worked out by hand from the rules - nothing here is computed by a copy of them, so a rule
change fails test_norm_geometry.py on a machine without a GPU and says which point no longer reaches its route.

The rules, for reference (BLOCK = 256 threads):
  one launch   vec4, N > 0 and B * ncg <= 512, with GC = 64 (C >= 256) / 32 (C >= 128) / 16 columns per group, ncg = ceil(C / GC),
               a block covers 8 * RLN rows per chunk, RLN = 256 / (GC / 4) = 16 / 32 / 64;  R = ceil((N div B) / (8 RLN)), at most
               ceil(2 cu / (B ncg)), at most (max(B, 1024) C div (ncg GC)) div B, at least 1 - and where that "at least 1" would
               not fit the workspace (C = 4, B > 256, two outputs) the call takes the two-stage route;
  two stages   4 or 1 channels per lane, CG = min(C / VW, 256) column lanes, RL = 256 div CG row lanes, 8 RL rows per chunk,
               nch = ceil((N div B) / (8 RL)) within 1 .. max(1, 1024 div B).
"""
import collections
import ctypes

ONE, TWO = 1, 2                               # STIN_COLREDUCE_ONE_LAUNCH / _TWO_STAGE (checked against the header by the CPU test)
E_SIZE, E_UNSUPPORTED, E_NULL = -2, -5, -1

# (id, N, C, B, nout, vec4, f32_rows) -> {cu: (family, width, chunks, (gx, gy, gz), partial doubles, ncg)} or an error code
Route = collections.namedtuple('Route', 'id N C B nout vec f32 want')


def _both(v):
    return {256: v, 64: v}


ROUTES = [
    # ---- one launch, GC = 16 (C < 128): 512 rows per chunk
    Route('t16-one-chunk', 512, 16, 1, 1, 1, 1, _both((ONE, 16, 1, (1, 1, 1), 16, 1))),
    Route('t16-second-chunk', 513, 16, 1, 2, 1, 1, _both((ONE, 16, 2, (2, 1, 1), 64, 1))),
    Route('t16-dead-lanes-c20', 700, 20, 1, 2, 1, 1, _both((ONE, 16, 2, (2, 2, 1), 128, 2))),
    Route('t16-cu-cap', 10 ** 6, 16, 1, 1, 1, 1, {256: (ONE, 16, 512, (512, 1, 1), 8192, 1), 64: (ONE, 16, 128, (128, 1, 1), 2048, 1)}),
    Route('t16-bf16-rows', 513, 16, 1, 2, 1, 0, _both((ONE, 16, 2, (2, 1, 1), 64, 1))),
    Route('t16-last-below-gc32', 513, 124, 1, 1, 1, 1, _both((ONE, 16, 2, (2, 8, 1), 256, 8))),
    # ---- C = 4: a column group is four times as wide as the matrix, the workspace bound bites first
    Route('c4-ws-bound-below', 100000, 4, 1, 2, 1, 1, {256: (ONE, 16, 196, (196, 1, 1), 6272, 1), 64: (ONE, 16, 128, (128, 1, 1), 4096, 1)}),
    Route('c4-ws-bound-256-chunks', 200000, 4, 1, 2, 1, 1, {256: (ONE, 16, 256, (256, 1, 1), 8192, 1), 64: (ONE, 16, 128, (128, 1, 1), 4096, 1)}),
    Route('c4-b256-two-outputs-fill-it', 2560, 4, 256, 2, 1, 1, _both((ONE, 16, 1, (1, 1, 256), 8192, 1))),
    Route('c4-b257-two-outputs-two-stage', 2570, 4, 257, 2, 1, 1, _both((TWO, 4, 1, (1, 257, 1), 2056, 0))),
    Route('c4-b300-two-outputs-two-stage', 3000, 4, 300, 2, 1, 1, _both((TWO, 4, 1, (1, 300, 1), 2400, 0))),
    Route('c4-b300-one-output-stays', 3000, 4, 300, 1, 1, 1, _both((ONE, 16, 1, (1, 1, 300), 4800, 1))),
    Route('c4-b512-two-outputs-two-stage', 5120, 4, 512, 2, 1, 1, _both((TWO, 4, 1, (1, 512, 1), 4096, 0))),
    Route('c4-b512-one-output-fills-it', 5120, 4, 512, 1, 1, 1, _both((ONE, 16, 1, (1, 1, 512), 8192, 1))),
    Route('c8-b512-two-outputs-fill-it', 5120, 8, 512, 2, 1, 1, _both((ONE, 16, 1, (1, 1, 512), 16384, 1))),
    # ---- GC = 32 (128 <= C < 256): 256 rows per chunk;  GC = 64 (C >= 256): 128 rows per chunk
    Route('t32-first', 257, 128, 1, 2, 1, 1, _both((ONE, 32, 2, (2, 4, 1), 512, 4))),
    Route('t32-dead-lanes-c132', 256, 132, 1, 1, 1, 1, _both((ONE, 32, 1, (1, 5, 1), 160, 5))),
    Route('t32-last', 257, 252, 1, 1, 1, 1, _both((ONE, 32, 2, (2, 8, 1), 512, 8))),
    Route('t64-first', 129, 256, 1, 2, 1, 1, _both((ONE, 64, 2, (2, 4, 1), 1024, 4))),
    Route('t64-dead-lanes-c260', 128, 260, 1, 2, 1, 1, _both((ONE, 64, 1, (1, 5, 1), 640, 5))),
    Route('t64-cu-cap', 10 ** 6, 256, 1, 2, 1, 1, {256: (ONE, 64, 128, (128, 4, 1), 65536, 4), 64: (ONE, 64, 32, (32, 4, 1), 16384, 4)}),
    Route('t64-c512-cu-cap', 10 ** 6, 512, 1, 1, 1, 1, {256: (ONE, 64, 64, (64, 8, 1), 32768, 8), 64: (ONE, 64, 16, (16, 8, 1), 8192, 8)}),
    # ---- the row of ticket words: B * ncg <= 512
    Route('words-512', 512 * 700, 16, 512, 2, 1, 1, _both((ONE, 16, 1, (1, 1, 512), 16384, 1))),
    Route('words-513', 513 * 700, 16, 513, 2, 1, 1, _both((TWO, 4, 1, (1, 513, 1), 16416, 0))),
    Route('words-516-seven-chunks', 129 * 1000, 64, 129, 2, 1, 1, _both((TWO, 4, 7, (7, 129, 1), 115584, 0))),
    Route('words-514-b257-c32', 257 * 600, 32, 257, 1, 1, 1, _both((TWO, 4, 3, (3, 257, 1), 24672, 0))),
    # ---- no rows, more ranges than slabs
    Route('no-rows-vec', 0, 16, 1, 2, 1, 1, _both((TWO, 4, 1, (1, 1, 1), 32, 0))),
    Route('no-rows-scalar', 0, 3, 2, 1, 0, 1, _both((TWO, 1, 1, (1, 2, 1), 6, 0))),
    Route('b1025-one-chunk', 1025 * 5000, 32, 1025, 2, 1, 1, _both((TWO, 4, 1, (1, 1025, 1), 65600, 0))),
    Route('b8192', 8192 * 9, 1024, 8192, 2, 1, 1, _both((TWO, 4, 1, (1, 8192, 1), 16777216, 0))),
    # ---- one channel per lane (fp32 rows that are no 16-byte vectors)
    Route('scalar-c3', 1000, 3, 1, 2, 0, 1, _both((TWO, 1, 2, (2, 1, 1), 12, 0))),
    Route('scalar-c1', 2049, 1, 1, 1, 0, 1, _both((TWO, 1, 2, (2, 1, 1), 2, 0))),
    Route('scalar-c256-odd-pitch', 8 * 17, 256, 1, 2, 0, 1, _both((TWO, 1, 17, (17, 1, 1), 8704, 0))),
    Route('scalar-c256-chunk-cap', 8 * 1024 + 1, 256, 1, 1, 0, 1, _both((TWO, 1, 1024, (1024, 1, 1), 262144, 0))),
    Route('scalar-c1024', 64, 1024, 1, 1, 0, 1, _both((TWO, 1, 8, (8, 1, 1), 8192, 0))),
    # ---- refusals and argument errors
    Route('bf16-rows-without-vec4', 100, 6, 1, 1, 0, 0, _both(E_UNSUPPORTED)),
    Route('vec4-claimed-at-c6', 100, 6, 1, 1, 1, 1, _both(E_SIZE)),
    Route('three-outputs', 100, 8, 1, 3, 1, 1, _both(E_SIZE)),
    Route('no-ranges', 100, 8, 0, 1, 1, 1, _both(E_SIZE)),
    Route('negative-rows', -1, 8, 1, 1, 1, 1, _both(E_SIZE)),
]

# (id, C, element bytes, data_align bytes, per-group vectors on 16 bytes, ld_align elements) -> 8 / 4 / 1 / refusal
Lane = collections.namedtuple('Lane', 'id C elem data_align stats16 ld_align want')
LANES = [
    Lane('bf16-8wide', 256, 2, 16, 1, 8, 8),
    Lane('bf16-8wide-c8', 8, 2, 16, 1, 16, 8),
    Lane('bf16-rows-on-8-bytes', 256, 2, 8, 1, 8, 4),
    Lane('bf16-pitch-of-4', 256, 2, 16, 1, 4, 4),
    Lane('bf16-c12', 12, 2, 16, 1, 4, 4),
    Lane('bf16-c12-rows-on-8-bytes', 12, 2, 8, 1, 4, 4),
    Lane('bf16-rows-on-4-bytes-refused', 12, 2, 4, 1, 4, E_UNSUPPORTED),
    Lane('bf16-c6-refused', 6, 2, 16, 1, 2, E_UNSUPPORTED),
    Lane('bf16-pitch-of-2-refused', 8, 2, 16, 1, 2, E_UNSUPPORTED),
    Lane('bf16-unaligned-statistics-refused', 256, 2, 16, 0, 8, E_UNSUPPORTED),
    Lane('f32-never-8wide', 256, 4, 16, 1, 8, 4),
    Lane('f32-c20', 20, 4, 16, 1, 4, 4),
    Lane('f32-c4', 4, 4, 16, 1, 4, 4),
    Lane('f32-rows-on-8-bytes', 256, 4, 8, 1, 4, 1),
    Lane('f32-one-float-off', 256, 4, 4, 1, 4, 1),
    Lane('f32-odd-pitch', 256, 4, 16, 1, 1, 1),
    Lane('f32-pitch-of-2', 256, 4, 16, 1, 2, 1),
    Lane('f32-c3', 3, 4, 16, 1, 1, 1),
    Lane('f32-c1', 1, 4, 16, 1, 4, 1),
    Lane('f32-unaligned-statistics', 256, 4, 16, 0, 4, 1),
]

KEYS = ('family', 'width', 'chunks', 'gx', 'gy', 'gz', 'partial', 'ncg')


def route(lib, N, C, B, nout, vec, f32, cu):
    """stin_colreduce_route -> (rc, dict of KEYS); a refusal leaves every value at -77"""
    out = (ctypes.c_int64 * 8)(*([-77] * 8))
    rc = lib.stin_colreduce_route(N, C, B, nout, vec, f32, cu, ctypes.addressof(out))
    return rc, dict(zip(KEYS, out))


def rows_for_chunks(C, R):
    """The smallest N (one range) whose one-launch reduction over C channels wants R row chunks"""
    rln = 256 // ((64 if C >= 256 else 32 if C >= 128 else 16) // 4)
    return (R - 1) * 8 * rln + 1
