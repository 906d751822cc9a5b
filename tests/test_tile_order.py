"""CPU: the sampling kernels' tile order as the host sees it (mpiv_tile_order, the kernels' own
xcd_tile_order compiled for the host).

Position t of the XCD-contiguous tile numbering belongs to XCD x when t lies in the x-th of eight
contiguous ranges of [0, ntiles), the first ntiles % 8 of them one longer.  The band order is the
identity.  The interleaved order is a permutation under which every XCD holds its fair share of
every tile row (tiles_x / 8) and of every tile column (tile rows / 8), rounded down or up."""
import pytest

from mpi_vision_amd import _lib

TILES_X = [1, 3, 4, 8, 9, 16, 17, 64]
TILE_ROWS = [1, 2, 3, 5, 7, 8, 9, 11, 16, 23, 43]  # ntiles < 8 and ntiles % 8 != 0 among them


def xcd_of(t, ntiles):
    q, r = ntiles >> 3, ntiles & 7
    return t // (q + 1) if t < r * (q + 1) else r + (t - r * (q + 1)) // max(q, 1)


@pytest.mark.parametrize("tiles_x", TILES_X)
def test_permutation_and_identity(tiles_x):
    for rows in TILE_ROWS:
        n = tiles_x * rows
        assert _lib.tile_order(n, tiles_x, -1) == list(range(n)), (tiles_x, rows)
        assert sorted(_lib.tile_order(n, tiles_x, 1)) == list(range(n)), (tiles_x, rows)
    assert any(tiles_x * rows < 8 for rows in TILE_ROWS) or tiles_x >= 8
    assert any(tiles_x * rows % 8 for rows in TILE_ROWS) or tiles_x % 8 == 0


@pytest.mark.parametrize("tiles_x", TILES_X)
def test_every_xcd_has_a_fair_share_of_rows_and_columns(tiles_x):
    for rows in TILE_ROWS:
        n = tiles_x * rows
        order = _lib.tile_order(n, tiles_x, 1)
        in_row, in_col = {}, {}
        for t, tile in enumerate(order):
            x = xcd_of(t, n)
            assert 0 <= x < 8
            in_row[x, tile // tiles_x] = in_row.get((x, tile // tiles_x), 0) + 1
            in_col[x, tile % tiles_x] = in_col.get((x, tile % tiles_x), 0) + 1
        for x in range(8):
            for ty in range(rows):
                assert tiles_x // 8 <= in_row.get((x, ty), 0) <= -(-tiles_x // 8), (tiles_x, rows, x, ty)
            if rows >= 8:
                for tx in range(tiles_x):
                    assert rows // 8 <= in_col.get((x, tx), 0) <= -(-rows // 8), (tiles_x, rows, x, tx)


def test_xcd_of_a_tile_where_tiles_x_is_a_multiple_of_8():
    """tiles_x = 16 and 64 (configs 4, 2 and 5): the XCD of tile (tx, ty) is (tx + ty) % 8."""
    for tiles_x, rows in ((16, 43), (64, 5), (8, 5)):
        n = tiles_x * rows
        for t, tile in enumerate(_lib.tile_order(n, tiles_x, 1)):
            assert xcd_of(t, n) == (tile % tiles_x + tile // tiles_x) % 8


def test_bad_arguments():
    for args in ((0, 4, 1), (8, 0, 1), (10, 4, 1), (8, 4, 0), (8, 4, 2)):
        with pytest.raises(RuntimeError, match="mpiv_tile_order"):
            _lib.tile_order(*args)
