"""WebP inputs on the MI355X, the stream shapes libwebp's encoder never writes: the cases of tests/test_webp_streams_emul.py through the product library
(decoder pinned to libwebp via Pillow).  What only the device runs -- the parse walked by a whole wave, the reconstruction's 64 scratch slots with rows 64
apart in flight, the prefix-code groups' slots in LDS, the predictor's and the alpha unfilter's wave fronts -- is held by these, not by the emulation."""
import pytest

import test_webp_streams_emul as E
from _util import product_api

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900, method="thread")]


@pytest.fixture(scope="module")
def api():
    a = product_api()
    assert a.device_count() >= 1, "no HIP device: libcaesium_hip has no CPU path"
    return a


def test_vp8_filter_types_levels_and_sharpness(api):
    E.test_emul_vp8_filter_types_levels_and_sharpness(api)


def test_vp8_filter_deltas(api):
    E.test_emul_vp8_filter_deltas(api)


def test_vp8_token_partitions(api):
    E.test_emul_vp8_token_partitions(api)


def test_vp8_segments(api):
    E.test_emul_vp8_segments(api)


def test_vp8_quantiser_index_deltas(api):
    E.test_emul_vp8_quantiser_index_deltas(api)


def test_vp8_skip_flag_and_empty_macroblocks(api):
    E.test_emul_vp8_skip_flag_and_empty_macroblocks(api)


def test_vp8_coefficient_probability_updates(api):
    E.test_emul_vp8_coefficient_probability_updates(api)


def test_vp8_prediction_modes_at_the_edges(api):
    E.test_emul_vp8_prediction_modes_at_the_edges(api)


def test_vp8_libwebp_encoder_knobs(api):
    E.test_emul_vp8_libwebp_encoder_knobs(api)


def test_vp8_frame_wider_than_2048(api):
    E.test_emul_vp8_frame_wider_than_2048(api)


def test_vp8l_colliding_groups(api):
    E.test_emul_vp8l_colliding_groups(api)


def test_vp8l_groups_past_the_table_threshold(api):
    E.test_emul_vp8l_groups_past_the_table_threshold(api)


def test_vp8l_groups_past_the_arena(api):
    E.test_emul_vp8l_groups_past_the_arena(api)


def test_vp8l_cache_bits_and_meta_tile_bits(api):
    E.test_emul_vp8l_cache_bits_and_meta_tile_bits(api)


def test_vp8l_code_depths_and_description_forms(api):
    E.test_emul_vp8l_code_depths_and_description_forms(api)


def test_vp8l_transforms_in_every_order(api):
    E.test_emul_vp8l_transforms_in_every_order(api)


def test_vp8l_palette_sizes(api):
    E.test_emul_vp8l_palette_sizes(api)


def test_vp8l_transform_tile_bits(api):
    E.test_emul_vp8l_transform_tile_bits(api)


def test_vp8l_predictor_modes_at_the_edges(api):
    E.test_emul_vp8l_predictor_modes_at_the_edges(api)


def test_vp8l_copies_at_every_distance_code(api):
    E.test_emul_vp8l_copies_at_every_distance_code(api)


def test_alph_filters_and_methods(api):
    E.test_emul_alph_filters_and_methods(api)
