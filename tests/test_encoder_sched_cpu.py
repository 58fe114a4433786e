"""The tile rule of the Inception trunk's grouped launches (sbagan.inception_hip._group_tile) is a pure function of the
level's (M, Cout) list: checked at its thresholds, each with a single item of 64 output channels."""
import pytest


@pytest.mark.parametrize('M,tile', [(128 * 512, 5),      # 512 tiles of 128 rows
                                    (128 * 511, 3),      # 511 of 128 rows, 682 of 96
                                    (96 * 512, 3),       # 384 of 128 rows, 512 of 96
                                    (96 * 511, 1)])      # 384 of 128 rows, 511 of 96
def test_group_tile_rule(M, tile):
    """tile 5 if sum ceil(M/128) ceil(Cout/64) >= 512, else tile 3 if sum ceil(M/96) ceil(Cout/64) >= 512, else tile 1"""
    from sbagan.inception_hip import _group_tile
    assert _group_tile([(M, 64)]) == tile
