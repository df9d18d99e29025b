"""The column cut of the fused layer kernels (include/mgcn_hip.h (2b) "Column cut", csrc/fused_common.h: fused_cut) through
mgcn_fused_cut: no device work. For every width the kernels take the chunks start on k-blocks (32 columns), cover the columns
once and in order, none is wider than 128; the widths outside 128 < D <= 256 keep the legacy chunks; D = 200 is cut 96 | 104;
and the modelled lines of a row are never above the legacy walk's. The model is recomputed here in Python from its definition."""
from math import gcd

import pytest

WIDTHS = list(range(4, 1025, 4))


def _model_lines(D, chunks, idle_col):
    """Mean 128-byte lines per row and mode: rows 4 D bytes apart start at every multiple of gcd(4 D, 128) within a line; a chunk
    touches the lines of its bytes, plus the line of the float4 its idle lanes load (idle_col(first, width)) where it has idle lanes
    and that line is none of them."""
    g = gcd(4 * D, 128)
    total = 0
    for o in range(0, 128, g):
        for c0, n in chunks:
            lo, hi = (o + 4 * c0) >> 7, (o + 4 * (c0 + n) - 1) >> 7
            total += hi - lo + 1
            il = (o + 4 * idle_col(c0, n)) >> 7
            if n < 128 and not lo <= il <= hi:
                total += 1
    return total / (128 // g)


def _legacy(D):
    return [(c, min(128, D - c)) for c in range(0, D, 128)]


def test_every_width_is_covered_once_on_k_block_boundaries(pkg):
    nat = pkg._native
    for D in WIDTHS:
        for legacy in (False, True):
            chunks, lines = nat.fused_cut(D, legacy)
            assert chunks[0][0] == 0 and sum(n for _, n in chunks) == D, (D, chunks)
            for (c0, n), nxt in zip(chunks, chunks[1:] + [(D, 0)]):
                assert c0 % 32 == 0 and 0 < n <= 128 and n % 4 == 0 and c0 + n == nxt[0], (D, chunks)
            idle = (lambda c0, n: 0) if legacy else (lambda c0, n: c0 + n - 4)
            assert lines == pytest.approx(_model_lines(D, chunks, idle), abs=1e-12), (D, legacy)
        assert nat.fused_cut(D, True)[0] == _legacy(D)


def test_todays_cut_outside_the_two_chunk_widths(pkg):
    nat = pkg._native
    for D in WIDTHS:
        if D <= 128 or D % 128 == 0 or D > 256:
            assert nat.fused_cut(D)[0] == _legacy(D), D
    assert nat.fused_cut(200)[0] == [(0, 96), (96, 104)]
    assert nat.fused_cut(200, legacy=True)[0] == [(0, 128), (128, 72)]
    assert nat.fused_cut(256)[0] == [(0, 128), (128, 128)]
    assert nat.fused_cut(228)[0] == [(0, 128), (128, 100)]            # 100 columns past 128: no other boundary leaves <= 128


def test_modelled_lines_never_above_the_legacy_walk(pkg):
    nat = pkg._native
    for D in WIDTHS:
        new, old = nat.fused_cut(D)[1], nat.fused_cut(D, True)[1]
        assert new <= old, (D, new, old)
        # ... and, for the widths with a choice, at the minimum over the boundaries on k-blocks (idle lanes inside their chunk)
        if 128 < D <= 256:
            best = min(_model_lines(D, [(0, b), (b, D - b)], lambda c0, n: c0 + n - 4) for b in (32, 64, 96, 128) if 0 < D - b <= 128)
            assert new == pytest.approx(best, abs=1e-12), D
    assert nat.fused_cut(200)[1] == pytest.approx(7.75) and nat.fused_cut(200, True)[1] == pytest.approx(8.75)


def test_widths_no_kernel_takes_are_refused(pkg):
    nat = pkg._native
    for D in (0, -4, 6, 1028):
        with pytest.raises(nat.NativeError):
            nat.fused_cut(D)
    assert nat.lib().mgcn_fused_cut(200, 0, None, None, 0, None) == 2   # the count alone
