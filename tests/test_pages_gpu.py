"""Whole pages on the MI355X: qea_page_tiles_gather / qea_page_tiles_scatter (csrc/page_tiles.hip) bit for bit against their
specification (qea/pages.py), the tiled pass against the fp64 oracle with the whole-page device pass as the yardstick, and the two front
ends (eval_prep.py --tile, clean_cli.py)."""
import numpy as np
import pytest
import torch

from test_pages_cpu import probe_values, seeded_page

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (17, 33), (437, 531), (400, 512)]


def _store(sizes, dtype, seed=11):
    """pages of `sizes` in one store with junk between them, every page at an ODD element offset -> (store, offset, h, w, pages)"""
    g = torch.Generator().manual_seed(seed)
    offset, off = [], 1
    for hh, ww in sizes:
        off += 1 - off % 2
        offset.append(off)
        off += hh * ww + 3
    if dtype == torch.uint8:
        store = torch.randint(0, 256, (off,), generator=g, dtype=torch.uint8)
    else:
        store = torch.rand(off, generator=g) * 1.5 - 0.25
    pages = [store[o:o + hh * ww].view(hh, ww) for o, (hh, ww) in zip(offset, sizes)]
    return store, np.asarray(offset, np.int64), np.asarray([s[0] for s in sizes], np.int32), np.asarray([s[1] for s in sizes], np.int32), pages


def _up(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).cuda()


GATHER_ROWS = {
    (320, 320): [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 0, 224), (2, 128, 0), (2, 128, 224), (3, 0, 0), (3, 80, 192), (2, 432, 528), (1, -16, -4),
                 (3, 399, 511), (2, 448, 0)],
    (48, 208): [(0, 0, 0), (1, 0, 0), (2, 400, 416), (3, 352, 304), (2, 16, 112), (3, 0, 0), (2, 389, 323), (1, -47, -207), (3, 352, 496)],
}


@pytest.mark.parametrize("shape", sorted(GATHER_ROWS))
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_gather_is_the_specification_bit_for_bit(dtype, shape):
    """Four pages (1x1, 17x33, 437x531, 400x512) in one store at odd offsets, tiles of all four in ONE launch, the 8-bit and the fp32 form:
    torch.equal with tiles_gather_spec, the white outside h x w included; a row that names no page gives a white tile."""
    from qea import ops
    from qea.pages import norm_table, tiles_gather_spec
    TH, TW = shape
    store, offset, h, w, _ = _store(SIZES, dtype)
    rows = np.asarray(GATHER_ROWS[shape], np.int32)
    want = tiles_gather_spec(store, offset, h, w, rows, TH, TW)
    assert want.dtype == torch.float32 and bool((want == 1).any()) and bool((want != 1).any())
    dev_rows = np.concatenate([rows, np.asarray([(4, 0, 0), (-1, 0, 0)], np.int32)])          # no such pages
    out = torch.full((len(dev_rows), 1, TH, TW), -7.0, device="cuda")
    before = ops.PAGE_LAUNCHES["gather"]
    ops.page_tiles_gather(_up(store), _up(offset), _up(h), _up(w), _up(dev_rows), out, norm_table().cuda() if dtype == torch.uint8 else None)
    assert ops.PAGE_LAUNCHES["gather"] == before + 1
    got = out.cpu()
    assert torch.equal(got[:len(rows)], want)
    assert bool((got[len(rows):] == 1).all())


def _probe_tiles(n, TH, TW):
    """n tiles whose elements walk through probe_values(), each tile from another start, so that every core holds every boundary"""
    v = probe_values()
    idx = (torch.arange(TH * TW)[None, :] * 7 + torch.arange(n)[:, None] * 131) % v.numel()
    return v[idx].view(n, 1, TH, TW).contiguous()


@pytest.mark.parametrize("which", ["both", "f32", "u8"])
@pytest.mark.parametrize("sizes,T", [(SIZES, 320), ([(33, 900), (5, 3)], 208)])
def test_scatter_is_the_specification_and_writes_every_pixel_once(sizes, T, which):
    """Outputs prefilled with a sentinel (0x5A / -7.0): after one launch per tile shape they equal tiles_scatter_spec on the same prefilled
    buffers everywhere — the junk between the pages is untouched — and no page pixel keeps its sentinel (the 8-bit output is also run from a
    second sentinel: a byte nobody wrote would differ between the two runs).  The tiles hold the values of the 8-bit rule's boundaries."""
    from qea import ops
    from qea.pages import plan_groups, tiles_scatter_spec
    _, offset, h, w, _ = _store(sizes, torch.uint8)
    n_el = int(offset[-1] + int(h[-1]) * int(w[-1]) + 3)
    groups = plan_groups(h, w, (T, T))
    tiles = {k: _probe_tiles(len(r), *k) for k, r in groups.items()}
    want_f, want_u = torch.full((n_el,), -7.0), torch.full((n_el,), 0x5A, dtype=torch.uint8)
    for k, r in groups.items():
        tiles_scatter_spec(tiles[k], r, offset, h, w, out_f=want_f, out_u8=want_u)
    d_off, d_h, d_w = _up(offset), _up(h), _up(w)

    def run(sentinel_u8):
        out_f = torch.full((n_el,), -7.0, device="cuda") if which != "u8" else None
        out_u = torch.full((n_el,), sentinel_u8, dtype=torch.uint8, device="cuda") if which != "f32" else None
        for k, r in groups.items():
            ops.page_tiles_scatter(tiles[k].cuda(), _up(r), d_off, d_h, d_w, out_f32=out_f, out_u8=out_u)
        return out_f, out_u
    out_f, out_u = run(0x5A)
    inside = torch.zeros(n_el, dtype=torch.bool)
    for o, hh, ww in zip(offset, h, w):
        inside[int(o):int(o) + int(hh) * int(ww)] = True
    if out_f is not None:
        assert torch.equal(out_f.cpu(), want_f)
        assert not bool((out_f.cpu()[inside] == -7.0).any()) and bool((out_f.cpu()[~inside] == -7.0).all())
    if out_u is not None:
        assert torch.equal(out_u.cpu(), want_u)
        again = run(0xA5)[1].cpu()
        assert torch.equal(again[inside], out_u.cpu()[inside]) and bool((again[~inside] == 0xA5).all()) and bool((out_u.cpu()[~inside] == 0x5A).all())


@pytest.fixture(scope="module")
def model():
    from models.model_unet import UNet
    from oracle import model_oracle as mo
    m = UNet()
    m.load_state_dict(mo.seeded_state(mo.unet_state_shapes(), 1))       # as tests/test_models_gpu.py::_load(UNet(), mo.unet_state_shapes, 1)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def oracle_whole():
    """page -> (padded page [1,1,Hp,Wp] fp32, the fp64 oracle's eval-mode pass over it [Hp,Wp]); computed once per page"""
    from oracle import model_oracle as mo
    P, Bf = mo.split_state({k: v.double() if v.is_floating_point() else v for k, v in mo.seeded_state(mo.unet_state_shapes(), 1).items()},
                           requires_grad=False)
    done = {}

    def whole(page):
        key = tuple(page.shape)
        if key not in done:
            hh, ww = page.shape
            padded = torch.ones(1, 1, (hh + 15) // 16 * 16, (ww + 15) // 16 * 16)
            padded[0, 0, :hh, :ww] = page
            with torch.no_grad():
                done[key] = (padded, mo.unet_forward(P, Bf, padded.double(), training=False)[0, 0])
        return done[key]
    return whole


def test_whole_path_against_the_oracle_with_the_whole_page_pass_as_yardstick(model, oracle_whole):
    """clean_pages on a 437x531 page with T = 320 (6 tiles) against the fp64 oracle's pass over the white-padded 448x544 page.  The yardstick
    is the error of the EXISTING whole-page device pass over that padded page against the same oracle: tiling changes only the per-tensor
    abs-max scales of the fp16 split, so the error class is the same — the tiled error may be at most twice that plus 1e-6 (a seam is 1e-3
    or more: tests/test_pages_cpu.py).  A batch of two pages gives per page what each page gives alone, within the same bound, and
    out="u8" is the quantised float result."""
    from qea.pages import clean_pages, quantise_u8
    pages = [seeded_page(437, 531, 7, torch.float32), seeded_page(350, 340, 8, torch.float32)]
    bounds, alone = [], []
    for page in pages:
        hh, ww = page.shape
        padded, want = oracle_whole(page)
        with torch.no_grad():
            e_whole = (model(padded.cuda())[0, 0].double().cpu() - want).abs().max().item()
        got = clean_pages(model, [page], tile=(320, 320))
        assert len(got) == 1 and got[0].shape == (hh, ww) and got[0].is_cuda and got[0].dtype == torch.float32
        e_tiled = (got[0].double().cpu() - want[:hh, :ww]).abs().max().item()
        print(f"{hh}x{ww}: whole-page device pass vs oracle {e_whole:.3g}, tiled (T = 320) vs oracle {e_tiled:.3g}")
        bounds.append(2 * e_whole + 1e-6)
        alone.append(got[0].cpu())
        assert e_tiled <= bounds[-1]
    both = clean_pages(model, pages, tile=(320, 320))                       # 6 + 4 tiles of 320 x 320 in one pass
    for page, b, a, bound in zip(pages, both, alone, bounds):
        hh, ww = page.shape
        e_batch = (b.double().cpu() - oracle_whole(page)[1][:hh, :ww]).abs().max().item()
        d_alone = (b.cpu() - a).abs().max().item()
        print(f"{hh}x{ww} in a batch of two: vs oracle {e_batch:.3g}, vs the page alone {d_alone:.3g}")
        assert e_batch <= bound and d_alone <= bound
    u8 = clean_pages(model, [pages[0][None]], tile=(320, 320), out="u8")
    assert u8[0].shape == (1, 437, 531) and u8[0].dtype == torch.uint8
    assert torch.equal(u8[0][0].cpu(), quantise_u8(alone[0]))
    # 8-bit pages in, a pass per tile (max_tile_pixels below one tile): the same plan, the same values
    page8 = quantise_u8(pages[1])
    a = clean_pages(model, [page8], tile=(320, 320), max_tile_pixels=1)[0]
    b = clean_pages(model, [page8.float() / 255], tile=(320, 320), max_tile_pixels=1)[0]
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="eval"):
        clean_pages(model.train(), pages, tile=(320, 320))
    model.eval()


def _docs():
    g = torch.Generator().manual_seed(4)
    boxes = [dict(label="ab", x_min=10, y_min=12, x_max=90, y_max=40), dict(label="cde", x_min=300, y_min=350, x_max=420, y_max=382),
             dict(label="f", x_min=480, y_min=380, x_max=512, y_max=400)]
    return [(torch.rand(1, 437, 531, generator=g), boxes, "odd/first.png"), (torch.rand(1, 400, 512, generator=g), boxes, "even/second.png")]


def test_eval_prep_tile_evaluates_documents_of_any_size(tmp_path):
    """--tile 320 320: both documents evaluate; without it the 437x531 document still raises the UNet's ValueError with its name."""
    from eval_prep import EvalPrep, build_parser
    from models.model_unet import UNet
    torch.save(UNet().cuda().eval(), tmp_path / "prep")
    base = ["--prep_path", str(tmp_path / "prep"), "--ocr", "stub"]
    acc, cer = EvalPrep(build_parser().parse_args(base + ["--tile", "320", "320"]), dataset=_docs()).eval()
    assert 0.0 <= acc <= 1.0 and cer >= 0.0
    with pytest.raises(ValueError, match="odd/first.png"):
        EvalPrep(build_parser().parse_args(base), dataset=_docs()).eval()


def test_clean_cli_writes_pages_of_the_same_sizes(tmp_path):
    """Two PNGs of different odd sizes in; out come PNGs of the same sizes and stems, mode L, with the bytes of clean_pages(..., out="u8")."""
    from PIL import Image
    import clean_cli
    from models.model_unet import UNet
    from qea.pages import clean_pages
    prep = UNet().cuda().eval()
    torch.save(prep, tmp_path / "prep")
    (tmp_path / "in").mkdir()
    g = torch.Generator().manual_seed(9)
    scans = {"b_scan": torch.randint(0, 256, (45, 67), generator=g, dtype=torch.uint8),
             "a_scan": torch.randint(0, 256, (233, 219), generator=g, dtype=torch.uint8)}
    for stem, px in scans.items():
        Image.fromarray(px.numpy()).save(tmp_path / "in" / f"{stem}.png")
    (tmp_path / "in" / "notes.txt").write_text("not an image")
    args = clean_cli.build_parser().parse_args(["--prep_path", str(tmp_path / "prep"), "--in_dir", str(tmp_path / "in"),
                                                "--out_dir", str(tmp_path / "out"), "--tile", "208", "208"])
    written = clean_cli.CleanPages(args).run()
    assert [p.split("/")[-1] for p in written] == ["a_scan.png", "b_scan.png"]
    want = clean_pages(prep, [scans["a_scan"], scans["b_scan"]], tile=(208, 208), out="u8")
    for path, w in zip(written, want):
        with Image.open(path) as img:
            assert img.mode == "L" and img.size == (w.shape[1], w.shape[0])
            assert np.array_equal(np.asarray(img), w.cpu().numpy())
