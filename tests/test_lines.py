"""CPU: the host specification of the windowed path for text lines of any width (tatt_amd/lines.py): the plan, the window stack, the
blend, the composition and the host halves of the two launches.  Everything here is integer arithmetic on uint8 once Pillow has resized
the line, so every comparison is exact."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import pil_resample_ref as R

LR = (16, 64)


def _img(seed, hs, ws, kind=1):
    return Image.fromarray(R.make_image(np.random.default_rng(seed), hs, ws, kind), "RGB")


# ---- line_plan ----------------------------------------------------------------------------------------------------------------------
def test_line_plan_examples():
    from tatt_amd import io
    assert io.line_plan((97, 16), LR, 32) == (97, [0, 32, 33])
    assert io.line_plan((65, 16), LR, 32) == (65, [0, 1])
    assert io.line_plan((128, 16), LR, 32) == (128, [0, 32, 64])
    assert io.line_plan((301, 23), LR, 32) == (209, [0, 32, 64, 96, 128, 145])     # 301 * 16 / 23 = 209.39
    assert io.line_plan((3, 2), LR, 32)[0] == 64 and io.line_plan((100, 32), LR, 32) == (64, [0])
    assert io.line_plan((9, 2), LR, 32)[0] == 72 and io.line_plan((129, 32), LR, 32)[0] == 65     # halves round up: 64.5 -> 65


def test_line_plan_gives_one_window_up_to_four_to_one():
    from tatt_amd import io
    for hs in (1, 7, 16, 23, 40, 200):
        for ws in (1, hs, 2 * hs, 4 * hs - 1, 4 * hs):
            assert io.line_plan((ws, hs), LR, 32) == (64, [0]), (ws, hs)
    assert io.line_plan((4 * 40 + 2, 40), LR, 32)[0] == 65


@pytest.mark.parametrize("stride", (32, 40, 48, 64))
def test_line_plan_covers_every_column_one_to_three_times(stride):
    from tatt_amd import io
    for wl in list(range(64, 400)) + [777, 1000, 2047, 2048, io.LINE_MAX_WL]:
        got, starts = io.line_plan((wl, 16), LR, stride)
        assert got == wl and starts[0] == 0 and starts[-1] == wl - 64
        assert all(b > a for a, b in zip(starts, starts[1:])), (wl, starts)
        assert starts[:-1] == [k * stride for k in range(len(starts) - 1)]
        cover = np.zeros(wl, int)
        for x in starts:
            cover[x:x + 64] += 1
        assert cover.min() >= 1 and cover.max() <= 3, (wl, stride, cover.min(), cover.max())


def test_line_plan_refuses_bad_strides_and_lines_beyond_the_limit():
    from tatt_amd import io
    for stride in (31, 65, 0, -32, 32.0):
        with pytest.raises(ValueError):
            io.line_plan((300, 16), LR, stride)
    assert io.LINE_MAX_WL >= 2048
    io.line_plan((io.LINE_MAX_WL, 16), LR, 32)
    with pytest.raises(ValueError):
        io.line_plan((io.LINE_MAX_WL + 1, 16), LR, 32)
    with pytest.raises(ValueError):
        io.line_plan((0, 16), LR, 32)


# ---- line_windows_host --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", (True, False))
def test_windows_are_training_crops_of_the_resized_line(mask):
    """every window equals resize_normalize of the window's crop of the ALREADY resized line: the mask threshold is the window's own"""
    from tatt_amd import io
    for seed, (hs, ws) in enumerate(((16, 97), (23, 301), (9, 40), (40, 500))):
        img = _img(seed, hs, ws, kind=2 if seed % 2 else 0)
        wl, starts = io.line_plan(img.size, LR, 32)
        line = img.resize((wl, 16), Image.BICUBIC)
        want = torch.stack([io.resize_normalize(line.crop((x, 0, x + 64, 16)), (64, 16), mask) for x in starts])
        got = io.line_windows_host(img, LR, 32, mask)
        assert got.shape == (len(starts), 3 + mask, 16, 64) and torch.equal(got, want)
    if mask:                                                         # dark left half, bright right half: the line's mean would differ
        a = np.full((16, 256, 3), 200, np.uint8)
        a[:, :128] = 20
        a[4:12, 10:20] = 5
        a[4:12, 200:220] = 120
        got = io.line_windows_host(Image.fromarray(a, "RGB"), LR, 64, True)
        assert got.shape[0] == 4 and 0 < float(got[0, 3].mean()) < 1 and 0 < float(got[3, 3].mean()) < 1


@pytest.mark.parametrize("mask", (True, False))
def test_one_window_is_resize_normalize(mask):
    from tatt_amd import io
    for seed, (hs, ws) in enumerate(((16, 64), (9, 30), (31, 120), (50, 37))):
        img = _img(10 + seed, hs, ws, kind=seed % 3)
        assert io.line_plan(img.size, LR, 32) == (64, [0])
        assert torch.equal(io.line_windows_host(img, LR, 32, mask), io.resize_normalize(img, (64, 16), mask)[None])


# ---- blend_windows_host -------------------------------------------------------------------------------------------------------------
def _blend_loop(q, starts, wl, scale):
    """the plain per-pixel statement: q (n, H, W, 3) uint8 windows -> (H, scale * wl, 3) uint8"""
    n, H, W, _ = q.shape
    out = np.zeros((H, scale * wl, 3), np.uint8)
    for y in range(H):
        for X in range(scale * wl):
            for c in range(3):
                N = D = 0
                for k, x in enumerate(starts):
                    j = X - scale * x
                    if 0 <= j < W:
                        wt = min(j + 1, W - j)
                        N += wt * int(q[k, y, j, c])
                        D += wt
                out[y, X, c] = (2 * N + D) // (2 * D)
    return out


@pytest.mark.parametrize("wl", (64, 65, 97, 128))
def test_blend_equals_the_per_pixel_loop(wl):
    from tatt_amd import io
    _, starts = io.line_plan((wl, 16), LR, 32)
    H, W = 4, 128                                                     # (4 rows keep the Python loop short: rows are independent)
    rng = np.random.default_rng(wl)
    q = rng.integers(0, 256, (len(starts), H, W, 4), dtype=np.uint8)
    sr = torch.from_numpy(q.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255))
    for c0 in (0, 1):
        got = io.blend_windows_host(sr, starts, wl, 2, "floor", c0)
        assert got.dtype == np.uint8 and got.shape == (H, 2 * wl, 3)
        assert np.array_equal(got, _blend_loop(q[..., c0:c0 + 3], starts, wl, 2))


@pytest.mark.parametrize("rule", ("floor", "round"))
def test_blend_of_one_window_is_its_quantisation(rule):
    from tatt_amd import io
    sr = torch.rand(1, 4, 32, 128, generator=torch.Generator().manual_seed(3)) * 1.4 - 0.2
    sr[0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0])
    want = io.quantize_u8(np.transpose(sr[0, :3].numpy(), (1, 2, 0)), rule)
    assert np.array_equal(io.blend_windows_host(sr, [0], 64, 2, rule), want)
    assert np.array_equal(io.blend_windows_host(sr, [0], 64, 2, rule), np.asarray(io.export_pil_batch(sr, None, rule)[0]))


def test_blend_of_identical_windows_is_the_constant():
    from tatt_amd import io
    for wl in (65, 97, 128, 209):
        _, starts = io.line_plan((wl, 16), LR, 32)
        for v in (0, 1, 127, 254, 255):
            sr = torch.full((len(starts), 3, 32, 128), v / 255.0)
            assert (io.blend_windows_host(sr, starts, wl, 2) == v).all(), (wl, v)


def test_blend_refuses_what_is_no_line():
    from tatt_amd import io
    sr = torch.zeros(2, 3, 32, 128)
    io.blend_windows_host(sr, [0, 1], 65, 2)
    for starts, wl, scale in (([0, 1], 65, 3), ([0, 2], 65, 2), ([1, 1], 65, 2), ([0], 65, 2), ([0, 80], 144, 2), ([0, 1], 65, 0)):
        with pytest.raises(ValueError):
            io.blend_windows_host(sr, starts, wl, scale)
    with pytest.raises(ValueError):
        io.blend_windows_host(sr, [0, 1], 65, 2, rule="nearest")
    with pytest.raises(ValueError):
        io.blend_windows_host(sr, [0, 1], 65, 2, c0=1)


def test_host_composition():
    """an identity-like 'model' (nearest-neighbour 2x of the RGB planes): sizes, the one-window case, out_sizes"""
    from tatt_amd import io
    up = lambda x: x[:, :3].repeat_interleave(2, 2).repeat_interleave(2, 3)
    imgs = [_img(1, 16, 64), _img(2, 23, 301, 0), _img(3, 9, 40, 2)]
    got = io.super_resolve_lines_host(imgs, up, LR, 32, True, "floor")
    assert [g.size for g in got] == [(128, 32), (418, 32), (142, 32)] and all(g.mode == "RGB" for g in got)
    assert np.array_equal(np.asarray(got[0]), np.asarray(imgs[0]).repeat(2, 0).repeat(2, 1))
    sized = io.super_resolve_lines_host(imgs, up, LR, 32, True, "floor", out_sizes=[(128, 32), (602, 46), (80, 18)])
    assert [g.size for g in sized] == [(128, 32), (602, 46), (80, 18)]
    assert np.array_equal(np.asarray(sized[1]), np.asarray(got[1].resize((602, 46), Image.BICUBIC)))
    with pytest.raises(ValueError):
        io.super_resolve_lines_host(imgs, lambda x: x[:, :3].repeat_interleave(2, 3), LR)


# ---- the host halves of the launches ------------------------------------------------------------------------------------------------
def test_line_limits_need_no_gpu():
    from tatt_amd import io
    lim = io.line_limits()
    assert set(lim) == {"rows", "cols", "wl", "h", "w", "inter_bytes", "table_bytes", "windows"}
    assert lim["wl"] == io.LINE_MAX_WL >= 2048 and lim["h"] >= 16 and lim["w"] >= 64 and lim["rows"] >= 64 and lim["cols"] >= 2048
    assert lim["windows"] >= len(io.line_plan((io.LINE_MAX_WL, 16), LR, 32)[1])


def test_lines_plan_rows_and_the_host_resize_fallback():
    from tatt_amd import io
    lim = io.line_limits()
    tall = _img(5, lim["rows"] + 44, 4000, 0)                        # beyond the source rows: PIL resizes the line on the host
    imgs = [_img(4, 23, 301), tall, _img(6, 16, 64)]
    arrays, desc, lines, nbytes, out_floats = io.lines_plan(imgs, LR, 32, True, lim)
    plans = [io.line_plan(im.size, LR, 32) for im in imgs]
    assert [(ln.wl, ln.starts) for ln in lines] == plans
    assert [ln.first for ln in lines] == [0, 6, 6 + len(plans[1][1])]
    n = sum(len(p[1]) for p in plans)
    assert desc.shape == (n, 12) and desc.dtype == np.int32 and out_floats == n * 4 * 16 * 64
    assert arrays[0].shape == (23, 301, 3) and arrays[2].shape == (16, 64, 3)
    wl = plans[1][0]
    assert arrays[1].shape == (16, wl, 3) and np.array_equal(arrays[1], np.asarray(tall.resize((wl, 16), Image.BICUBIC)))
    for ln, a in zip(lines, arrays):
        rows = desc[ln.first:ln.first + len(ln.starts)]
        assert len(set(rows[:, 0].tolist())) == 1 and int(rows[0, 0]) % 16 == 0            # one upload per line
        assert (rows[:, 1:3] == a.shape[:2]).all() and (rows[:, 3] == 16).all() and (rows[:, 4] == ln.wl).all()
        assert rows[:, 5].tolist() == ln.starts and (rows[:, 6] == 64).all() and (rows[:, 7] == 1).all() and not rows[:, 9:].any()
    assert desc[:, 8].tolist() == [k * 4 * 16 * 64 for k in range(n)]
    assert nbytes >= sum(a.size for a in arrays)
    flat = np.zeros(io.lines_fill(None, arrays, desc)[1], np.uint8)
    pix, used = io.lines_fill(flat, arrays, desc)
    assert used == flat.size
    for ln, a in zip(lines, arrays):
        o = pix + int(desc[ln.first, 0])
        assert np.array_equal(flat[o:o + a.size], a.reshape(-1))
    # the same windows either way: cutting the host-resized line is what line_windows_host does
    want = io.line_windows_host(tall, LR, 32, True)
    line = Image.fromarray(arrays[1], "RGB")
    got = torch.stack([io.resize_normalize(line.crop((x, 0, x + 64, 16)), (64, 16), True) for x in lines[1].starts])
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        io.lines_plan([_img(7, 16, 64).convert("L")], LR, 32, True, lim)


def test_blend_plan_rows():
    from tatt_amd import io
    lines = [io.Line(209, io.line_plan((209, 16))[1], 0), io.Line(64, [0], 6), io.Line(65, [0, 1], 7)]
    desc, starts, nbytes = io.blend_plan(lines, 9, 32, 128, 2, "round", 1)
    assert desc.tolist() == [[0, 6, 209, 2, 1, 1, 0, 1254], [6, 1, 64, 2, 1, 1, 40128, 384], [7, 2, 65, 2, 1, 1, 52416, 390]]
    assert starts.tolist() == [0, 32, 64, 96, 128, 145, 0, 0, 1] and nbytes == 52416 + 32 * 390
    with pytest.raises(ValueError):
        io.blend_plan(lines, 10, 32, 128, 2)
    with pytest.raises(ValueError):
        io.blend_plan(lines[1:], 3, 32, 128, 2)
    with pytest.raises(ValueError):
        io.blend_plan(lines, 9, 32, 128, 4)


def test_super_resolver_has_no_cpu_path_for_lines():
    import tatt_amd
    from tatt_amd.infer import SuperResolver
    m = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=1, hidden_units=32)
    with pytest.raises(RuntimeError, match="GPU"):
        SuperResolver(m, long_lines=True)                            # (no CPU path, with or without the keyword)
