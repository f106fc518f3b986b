"""Hygiene of the shipped tile table (scrubvae_amd/tuned_tiles.json) on the host, without loading the library: every key rebuilds
the Conv it was tuned for, and every value is a code `Conv._tune` could have chosen for that key.  A hand-edited or re-tuned table that
ships a code the tuner never tries fails here; tests/test_gpu_tile_table.py runs every entry on the GPU."""
import pytest

from scrubvae_amd import ops


def parse_key(key):
    """Tile-table key -> (kind, base pieces, Conv).  Key layout: Conv.tile_key --
    kind[@pieces]:batch:l_in:c_in:c_out:ld_in:ld_out:kernel:stride:padding:transposed[:up2]."""
    f = key.split(":")
    kind, _, base = f[0].partition("@")
    base = int(base) if base else 0
    assert kind in ("fwd", "dgrad", "wgrad"), key
    assert len(f) in (11, 12) and (len(f) == 11 or f[11] == "up2"), key
    B, L, ci, co, ldi, ldo, k, s, p, tr = (int(v) for v in f[1:11])
    assert tr in (0, 1) and ci % 16 == 0 and co % 16 == 0 and ldi >= ci and ldo >= co, key
    cv = ops.Conv(B, L, ci, co, k, s, p, 1, bool(tr), ld_in=ldi, ld_out=ldo, pieces=base, up2=len(f) == 12)
    if kind == "dgrad":
        cv.dgrad_pieces = base
    elif kind == "wgrad":
        cv.wgrad_pieces = base
    return kind, base, cv


KEYS = sorted(ops.TILE_TABLE)


def test_table_is_the_shipped_one():
    assert len(KEYS) > 900  # tuned_tiles.json was found and read (an unreadable table only warns)


@pytest.mark.parametrize("key", KEYS)
def test_table_entry_is_a_tuner_candidate(key):
    kind, base, cv = parse_key(key)
    assert cv.tile_key(kind) == key
    v = int(ops.TILE_TABLE[key])
    flag = ops.Conv._F32_FLAG
    assert v > 0
    if v >= flag:  # the fp32 kernel for one pass of a split-precision conv
        assert base, f"{key}: fp32 flag on a key without split pieces"
        assert v < 2 * flag
        assert v % flag in (ops._WGRAD_CODES if kind == "wgrad" else ops._GATHER_CODES), (key, v)
    elif base:
        assert v in (ops._SPLIT_WGRAD_CODES if kind == "wgrad" else ops._SPLIT_GATHER_CODES), (key, v)
    else:
        assert v in (ops._WGRAD_CODES if kind == "wgrad" else ops._GATHER_CODES), (key, v)
