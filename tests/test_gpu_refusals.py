"""What the public entry points refuse on the host, before any launch: per entry point, the name the message starts with and the
phrase that tells one refusal from another.  Cornell at 33x8, depth 2.  Where several refusals apply to one call, the one pinned is
the one the library has always reported (the order of the checks is part of its behaviour).

An adaptive state on a partial-row tile cannot be reached (pt_adaptive_round refuses such a tile), so the combinations below pair the
refusals that can meet."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H = 33, 8
ROWS = "whole contiguous image rows"
TILES = {"partial": dict(pixel_begin=0, pixel_count=40),                                         # 40 is no multiple of 33
         "striped": dict(pixel_begin=0, pixel_count=2 * W, stripe_pixels=11, stripe_stride=W)}  # begin and count alone would pass


@pytest.fixture(scope="module")
def scene(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    sc = capi.Scene(scene_dir["cornell"], res=(W, H))
    sc.trace_depth = 2
    return sc


class renderer:
    def __init__(self, scene, **kw):
        self.scene, self.kw = scene, kw

    def __enter__(self):
        from cosc_4397_pathtracing_raytracing_project_amd import capi
        self.r = capi.Renderer(self.scene, iters_per_batch=2, **self.kw)
        return self.r

    def __exit__(self, *exc):
        self.r.free()


def refused(who, phrase, call, *args, **kw):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    with pytest.raises(capi.PtError) as e:
        call(*args, **kw)
    msg = str(e.value)
    assert msg.startswith(who + ": ") and phrase in msg, (who, phrase, msg)


@pytest.mark.parametrize("tile", sorted(TILES))
def test_tiles_that_are_not_whole_contiguous_rows(scene, tile):
    with renderer(scene, **TILES[tile]) as r:
        r.render(1, 1)
        refused("pt_denoise", ROWS, r.denoise, 1.0)
        refused("pt_denoise_guided", ROWS, r.denoise_guided)  # (no feature pass and nothing folded either: the rows come first)
        refused("pt_adaptive_round", ROWS, r.adaptive_round, 2, 1, 0.5)  # (0 groups folded as well)
        refused("pt_render_adaptive", ROWS, r.render_adaptive, 2, 2, 60.0, 0.5)
        refused("pt_render_adaptive", "fraction 2 is not in (0, 1]", r.render_adaptive, 2, 2, 60.0, 2.0)  # the arguments before the tile
        assert r.stats().samples == r.n  # nothing further was rendered


def test_save_u8_has_its_own_row_rule(scene):
    with renderer(scene, **TILES["partial"]) as r:
        refused("pt_save_u8", "whole image rows", r.save_u8, 1.0)
        refused("pt_save_u8", "samples must be positive", r.save_u8, 0.0)  # the argument before the tile
    with renderer(scene, **TILES["striped"]) as r:
        refused("pt_save_u8", "whole image rows", r.save_u8, 1.0)
    with renderer(scene, pixel_begin=W, pixel_count=2 * W, stripe_pixels=W, stripe_stride=2 * W) as r:  # rows 1 and 3
        r.render(1, 1)
        assert r.save_u8(1.0).shape == (2, W, 3)
        refused("pt_denoise", ROWS, r.denoise, 1.0)  # the filters want the rows contiguous as well


def test_adaptive_state(scene):
    ADAPTIVE = "adaptive state"
    with renderer(scene) as r:
        for first in (1, 3):
            r.render(first, 2)
            r.noise_fold()
        r.adaptive_round(5, 2, 0.25)
        refused("pt_render", ADAPTIVE, r.render, 7, 1)
        refused("pt_denoise", ADAPTIVE, r.denoise, 4.0)  # (no feature pass either: the state comes first)
        refused("pt_denoise_guided", ADAPTIVE, r.denoise_guided)
        refused("pt_noise_fold", ADAPTIVE, r.noise_fold)
        refused("pt_render_until", ADAPTIVE, r.render_until, 7, 2, 60.0)
        refused("pt_render_until", "the count >= 1", r.render_until, 7, 0, 60.0)  # the arguments before the state
        refused("pt_save_u8", ADAPTIVE, r.save_u8, 4.0)
        refused("pt_save_u8", "samples must be positive", r.save_u8, -1.0)  # the argument before the state
        refused("pt_preview_rgba8", ADAPTIVE, r.preview, 4)
        assert r.resolve().shape == (r.n, 3)  # how the adaptive state is read
        r.clear()  # back to the uniform state
        assert not r.readback_adaptive().any() and r.noise() == dict(sse=-1.0, groups=0, iterations=0)
        r.render(1, 1)
        r.noise_fold()
        assert r.save_u8(1.0).shape == (H, W, 3) and r.preview(1).shape == (r.n, 4)
        assert r.render_until(2, 2, 1e9, 1)[0] == 2
        assert r.stats().samples == 3 * r.n


def test_fold_state(scene):
    with renderer(scene) as r:
        r.render(1, 1)
        r.render_features(1, 1)
        # nothing folded, and an iteration rendered since: what is missing comes before what is stale
        refused("pt_denoise_guided", "nothing has been folded", r.denoise_guided)
        refused("pt_adaptive_round", "0 group(s) folded", r.adaptive_round, 2, 1, 0.5)
        refused("pt_resolve", "nothing has been folded", r.resolve)
        r.noise_fold()
        r.render(2, 1)
        refused("pt_adaptive_round", "1 group(s) folded", r.adaptive_round, 3, 1, 0.5)  # one group, and an iteration since
        refused("pt_denoise_guided", "fold first", r.denoise_guided)  # (one group is the filter's own refusal, after this one)
        refused("pt_resolve", "fold first", r.resolve)
        r.noise_fold()
        r.render(3, 1)
        for who, call, args in (("pt_denoise_guided", r.denoise_guided, ()), ("pt_adaptive_round", r.adaptive_round, (4, 1, 0.5)),
                                ("pt_resolve", r.resolve, ())):
            refused(who, "1 iteration(s) rendered since the last fold; fold first (pt_noise_fold)", call, *args)
        refused("pt_adaptive_round", "fraction 0 is not in (0, 1]", r.adaptive_round, 4, 1, 0.0)  # the arguments before the folds
        r.noise_fold()
        assert np.isfinite(r.denoise_guided()).all() and np.isfinite(r.resolve()).all()
        assert r.stats().samples == 3 * r.n
