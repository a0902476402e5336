"""Host-only A/B of the TN route answers of two builds of the library (no GPU is touched): stin_gemm_tn_geometry (the first eight
values), stin_gemm_tn_workspace_bytes, stin_edgeconv_wgrad_workspace_bytes and stin_edgeconv_wgrad_map_supported over a dense sweep
of shapes, row pitches, alignments and the three switches STIN_TN_WS / STIN_TN_BIG / STIN_TN_TR unset / 0 / 1.

    python profiles/probes/tn_route_probe.py <parent libstin_hip.so> <new libstin_hip.so>

Asserts: the eight geometry values, the error code of the query and map_supported are EQUAL at every point; every workspace value of
the new library holds the slabs of the new geometry at that point (the block bound: slab A in its part, slab B in the rest, for the
wide AND the compact layout of the packed product); stin_gemm_tn_workspace_bytes is never above the parent's.  Prints the number of points and the shapes
whose workspace bound shrank.
"""
import ctypes
import itertools
import os
import sys

WIDTHS = (3, 4, 10, 12, 16, 20, 28, 32, 36, 60, 64, 68, 72, 128, 132, 256, 260, 320, 512, 520, 1024, 1028)
ROWS = (0, 1, 127, 128, 129, 1153, 4097, 18063, 32768, 32769, 60211, 131072, 131073, 200704, 1200642)
PAD_ALIGNED = ((0, 1), (1, 1), (0, 0))
PRECISIONS = (0, 2, 3)                    # STIN_GEMM_F32 / _BF16X3 / _BF16X6
SWITCHES = ('STIN_TN_WS', 'STIN_TN_BIG', 'STIN_TN_TR')
I64, I32, P = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.stin_gemm_tn_geometry.argtypes = [I32, I64, I32, I32, I64, I64, I32, I32, I32, P]
    lib.stin_gemm_tn_geometry.restype = I32
    lib.stin_gemm_tn_workspace_bytes.argtypes = [I64, I32, I32, I32]
    lib.stin_gemm_tn_workspace_bytes.restype = ctypes.c_size_t
    lib.stin_edgeconv_wgrad_workspace_bytes.argtypes = [I64, I32, I32, I32, I32]
    lib.stin_edgeconv_wgrad_workspace_bytes.restype = ctypes.c_size_t
    lib.stin_edgeconv_wgrad_map_supported.argtypes = [I64, I32, I32, I32, I32, I32]
    lib.stin_edgeconv_wgrad_map_supported.restype = I32
    return lib


def geometry(lib, buf, *args):
    for i in range(10):
        buf[i] = -7
    rc = lib.stin_gemm_tn_geometry(*args, ctypes.addressof(buf))
    return rc, tuple(buf[:8])


def slab_bytes(chunks, Nc, K):
    return chunks * (Nc * ((K + 3) & ~3) + ((Nc + 3) & ~3)) * 4 + 256


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    buf = (ctypes.c_int32 * 10)()
    points = ws_points = 0
    shrank, grew = {}, []
    for env in itertools.product((None, '0', '1'), repeat=3):
        for k, v in zip(SWITCHES, env):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        for Nc, K, M in itertools.product(WIDTHS, WIDTHS, ROWS):
            need = 0                     # the largest slab of the NEW geometry over storage, precision, pitch and alignment
            for storage, prec, (pad, al) in itertools.product((0, 1), PRECISIONS, PAD_ALIGNED):
                args = (storage, M, Nc, K, Nc + pad, K + pad, al, 1, prec)
                a, b = geometry(old, buf, *args), geometry(new, buf, *args)
                assert a == b, (env, args, a, b)
                points += 1
                if b[0] == 0:
                    need = max(need, slab_bytes(b[1][5], Nc, K))
            for ones in (0, 1):
                wa, wb = old.stin_gemm_tn_workspace_bytes(M, Nc, K, ones), new.stin_gemm_tn_workspace_bytes(M, Nc, K, ones)
                assert need <= wb <= wa, (env, M, Nc, K, ones, need, wb, wa)
                ws_points += 1
                if wb < wa:
                    shrank.setdefault((Nc, K), []).append((M, wa, wb))
            # a block of Cp = K, H = Nc, Cout = Nc: products (M, Nc, Nc) and (M, Yw, K), Yw = 2 Nc (+ Nc) or, in the compact
            # trans-inv layout (fp32 rows), Nc (+ Nc).  The entry points lay slab A (rounded up to 256 bytes) in front of slab B
            # and guard each: A must fit its part of the bound, B the rest.
            for sc in (0, 1):
                wa = old.stin_edgeconv_wgrad_workspace_bytes(M, K, Nc, Nc, sc)
                wb = new.stin_edgeconv_wgrad_workspace_bytes(M, K, Nc, Nc, sc)
                off_b = (new.stin_gemm_tn_workspace_bytes(M, Nc, Nc, 1) + 255) // 256 * 256
                need_a = need_b = 0
                for Yw, storages in ((2 * Nc + (Nc if sc else 0), (0, 1)), (Nc + (Nc if sc else 0), (0,))):
                    for storage, prec, al in itertools.product(storages, PRECISIONS, (0, 1)):
                        ga = geometry(new, buf, storage, M, Nc, Nc, Nc, Nc + 4, al, 1, prec)
                        gb = geometry(new, buf, storage, M, Yw, K, Yw, K, al, 1, prec)
                        assert ga[0] == 0 and gb[0] == 0
                        need_a, need_b = max(need_a, slab_bytes(ga[1][5], Nc, Nc)), max(need_b, slab_bytes(gb[1][5], Yw, K))
                assert need_a <= off_b and off_b + need_b + 256 <= wb, (env, M, Nc, K, sc, need_a, off_b, need_b, wb)
                if wb > wa:
                    grew.append((M, K, Nc, sc, wa, wb))
                ws_points += 1
                for prec in PRECISIONS:
                    assert old.stin_edgeconv_wgrad_map_supported(M, K, Nc, Nc, sc, prec) == new.stin_edgeconv_wgrad_map_supported(M, K, Nc, Nc, sc, prec)
                    points += 1
    print('%d geometry / map_supported points equal, %d workspace values checked' % (points, ws_points))
    print('stin_edgeconv_wgrad_workspace_bytes above the parent\'s at %d points (N, Cp, H = Cout, shortcut, parent, new):' % len(grew))
    for g in grew[:40]:
        print('  ', g)
    print('stin_gemm_tn_workspace_bytes shrank at %d (Nc, K) shapes:' % len(shrank))
    for (Nc, K), rows in sorted(shrank.items()):
        ms = sorted({m for m, _, _ in rows})
        worst = max(rows, key=lambda r: r[1] - r[2])
        print('  Nc %4d K %4d  at M in %s  (largest: M = %d, %d -> %d bytes)' % (Nc, K, ms, worst[0], worst[1], worst[2]))


if __name__ == '__main__':
    main()
