"""Whole-page tiling on the host (qea/pages.py): the plan's properties, the stitched pass against the whole pass with the fp64 oracle
(and a too small halo showing its seam), the 8-bit rule of the scatter, the specifications of the two kernels of csrc/page_tiles.hip, the
library's two entry points, and the command-line surface."""
import numpy as np
import pytest
import torch

torch.set_num_threads(4)

LENGTHS = sorted(set(range(1, 1501, 2)) | set(range(16, 1501, 16)))


def probe_values():
    """fp32 values that hit every truncation boundary of the 8-bit rule: k / 255, its two fp32 neighbours, and 0, 1, -0.5, 1.5"""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    v = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-2)), np.float32([0, 1, -0.5, 1.5])])
    return torch.from_numpy(v.astype(np.float32))


def seeded_page(h, w, seed, dtype=torch.float64):
    return torch.rand(h, w, generator=torch.Generator().manual_seed(seed), dtype=dtype)


@pytest.mark.parametrize("T", [208, 320, 400, 1024])
def test_plan_axis_properties(T):
    from qea.pages import HALO, plan_axis
    assert HALO == 96
    for L in LENGTHS:
        Lp = (L + 15) // 16 * 16
        plan = plan_axis(L, T)
        assert plan[0][0] == 0 and plan[-1][0] + plan[-1][1] == Lp, (L, plan)
        end = 0
        for o, size, c0, c1 in plan:
            assert size == (Lp if Lp <= T else T) and o % 16 == 0 and c0 % 16 == 0 and c1 % 16 == 0, (L, plan)   # Lp itself is a multiple
            assert c0 == end and c0 < c1, (L, plan)                       # the cores partition [0, Lp): each starts where the last ended
            assert o <= c0 and c1 <= o + size, (L, plan)                  # ... and lies inside its tile
            assert c0 == 0 or c0 - o >= HALO, (L, plan)                   # an interior core side has HALO px of tile beyond it
            assert c1 == Lp or o + size - c1 >= HALO, (L, plan)
            end = c1
        assert end == Lp, (L, plan)


def test_plan_refuses_bad_tiles_and_is_a_product():
    from qea.pages import plan_axis, plan_tiles
    for T in (200, 330, 192):
        with pytest.raises(ValueError):
            plan_axis(500, T)
        with pytest.raises(ValueError):
            plan_tiles(500, 500, (320, T))
    TH, TW, rows = plan_tiles(437, 531, (320, 320))
    assert (TH, TW) == (320, 320) and len(rows) == 6
    ys, xs = plan_axis(437, 320), plan_axis(531, 320)
    assert rows == [(oy, ox, a, b, c, d) for oy, _, a, b in ys for ox, _, c, d in xs]
    assert plan_tiles(33, 900, (208, 208))[:2] == (48, 208) and len(plan_tiles(33, 900, (208, 208))[2]) == 45
    assert plan_tiles(1, 1, (1024, 1024)) == (16, 16, [(0, 0, 0, 16, 0, 16)])


@pytest.fixture(scope="module")
def oracle8():
    from oracle import model_oracle as mo
    P, Bf = mo.split_state({k: v.double() if v.is_floating_point() else v for k, v in mo.seeded_state(mo.unet_state_shapes(f=8), 5).items()},
                           requires_grad=False)

    def forward(x):
        with torch.no_grad():
            return mo.unet_forward(P, Bf, x, training=False)
    return forward


@pytest.mark.parametrize("h,w,T", [(437, 531, 320), (33, 900, 208)])
def test_stitched_equals_whole_and_a_short_halo_shows_its_seam(oracle8, h, w, T):
    """fp64 oracle, f = 8: the tiled pass is the whole pass over the white-padded page (measured 2.3e-15 / 1.7e-15; 1e-12 only covers another
    summation order at another shape), and the same call with halo = 80 is not (measured 1.1e-2): the test can see a seam."""
    from qea.pages import clean_pages_spec
    page = seeded_page(h, w, 7)
    hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    padded = torch.ones(1, 1, hp, wp, dtype=torch.float64)
    padded[0, 0, :h, :w] = page
    whole = oracle8(padded)[0, 0, :h, :w]
    got = clean_pages_spec(oracle8, [page], (T, T))
    assert len(got) == 1 and got[0].shape == (h, w) and got[0].dtype == torch.float64
    err = (got[0] - whole).abs().max().item()
    seam = (clean_pages_spec(oracle8, [page], (T, T), halo=80)[0] - whole).abs().max().item()
    print(f"{h}x{w} T={T}: stitched vs whole {err:.3g}, with halo 80 {seam:.3g}")
    assert err <= 1e-12
    assert seam > 1e-6


def test_u8_rule_of_the_scatter():
    """(uint8)(min(max(x, 0), 1) * 255): torch's expression, and the same in numpy fp32, on every truncation boundary; NaN gives 0."""
    from qea.pages import quantise_u8, tiles_scatter_spec
    v = probe_values()
    want = (v.clamp(0, 1) * 255).to(torch.uint8)
    assert torch.equal(quantise_u8(v), want)
    n = v.numpy()
    assert np.array_equal(want.numpy(), (np.clip(n, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8))
    assert want[-4:].tolist() == [0, 255, 0, 255] and want[255].item() == 255 and want[0].item() == 0
    assert quantise_u8(torch.tensor([float("nan"), 0.5])).tolist() == [0, 127]
    # ... and through the scatter's specification: a 32 x 48 tile whose core is the page
    tile = torch.ones(32 * 48)
    tile[:v.numel()] = v
    out = torch.full((32 * 48,), 0x5A, dtype=torch.uint8)
    tiles_scatter_spec(tile.view(1, 1, 32, 48), [(0, 0, 0, 0, 32, 0, 48)], [0], [32], [48], out_u8=out)
    assert torch.equal(out[:v.numel()], want) and bool((out[v.numel():] == 255).all())


def test_gather_and_scatter_specs_on_packed_pages():
    """pack_pages + the two specifications: white outside the page, uint8 through p / 255, cores pasted once, shapes and dims kept."""
    from qea.pages import clean_pages_spec, pack_pages, plan_groups, tiles_gather_spec, unpack_pages
    g = torch.Generator().manual_seed(3)
    pages = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in ((1, 1), (17, 33), (250, 40))]
    pk = pack_pages(pages)
    assert pk.offset.tolist() == [0, 1, 1 + 17 * 33] and pk.store.numel() == 1 + 17 * 33 + 250 * 40
    assert all(torch.equal(a, b) for a, b in zip(unpack_pages(pk.store, pk), pages))
    groups = plan_groups(pk.h, pk.w, (208, 208))
    assert list(groups) == [(16, 16), (32, 48), (208, 48)] and [len(r) for r in groups.values()] == [1, 1, 4]
    t = tiles_gather_spec(pk.store, pk.offset, pk.h, pk.w, groups[(32, 48)], 32, 48)
    assert t.shape == (1, 1, 32, 48) and t.dtype == torch.float32
    assert torch.equal(t[0, 0, :17, :33], pages[1].float() / 255) and bool((t[0, 0, 17:] == 1).all()) and bool((t[0, 0, :, 33:] == 1).all())
    # the identity as the model: every page comes back, as float (p / 255) and as 8-bit (exactly p: 255 * (p / 255) truncates to p ...
    same = clean_pages_spec(lambda x: x, pages, (208, 208))
    assert all(torch.equal(a, b.float() / 255) for a, b in zip(same, pages))
    back = clean_pages_spec(lambda x: x, pages, (208, 208), out="u8", max_tile_pixels=3 * 208 * 48)
    want = [(p.float() / 255 * 255).to(torch.uint8) for p in pages]         # ... or to p - 1 where the fp32 product falls just below)
    assert all(torch.equal(a, b) for a, b in zip(back, want))
    # float pages keep their dims; kinds do not mix
    f = clean_pages_spec(lambda x: x * 0.5, [torch.rand(1, 20, 30), torch.rand(40, 300)], (208, 208))
    assert f[0].shape == (1, 20, 30) and f[1].shape == (40, 300)
    with pytest.raises(ValueError):
        pack_pages([pages[0], torch.rand(4, 4)])
    with pytest.raises(ValueError):
        pack_pages([torch.rand(2, 4, 4)])


def test_clean_pages_refuses_train_mode_bad_tiles_and_runs_the_host_backend():
    from oracle.modules import OracleUNet
    from qea.pages import clean_pages, clean_pages_spec
    model = OracleUNet(seed=5)
    page = seeded_page(40, 230, 2, torch.float32)
    with pytest.raises(ValueError, match="eval"):
        clean_pages(model.train(), [page], tile=(208, 208))
    model.eval()
    for tile in ((200, 208), (208, 330), (192, 192)):
        with pytest.raises(ValueError):
            clean_pages(model, [page], tile=tile)
    with pytest.raises(ValueError):
        clean_pages(model, [page], tile=(208, 208), out="png")
    got = clean_pages(model, [page], tile=(208, 208), out="u8")
    with torch.no_grad():
        want = clean_pages_spec(lambda x: model(x), [page], (208, 208), out="u8")
    assert got[0].shape == (40, 230) and got[0].dtype == torch.uint8 and torch.equal(got[0], want[0])


def test_eval_prep_tile_on_the_host_backend(tmp_path):
    """The oracle injected as the backend: with --tile the area flow gives what it gives without (a 32x128 strip is one tile), and the patch
    flow evaluates a 45x150 document, whose sides are no multiples of 16."""
    from datasets.synthetic import SyntheticTextAreas
    from eval_prep import EvalPrep, build_parser
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.trainer_core import Backend
    backend = Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)
    torch.save(OracleUNet(seed=5).eval(), tmp_path / "prep")
    base = ["--prep_path", str(tmp_path / "prep"), "--ocr", "stub"]
    area = base + ["--dataset", "vgg", "--batch_size", "2"]
    va = SyntheticTextAreas(3, seed=2)
    plain = EvalPrep(build_parser().parse_args(area), backend=backend, dataset=va).eval()
    tiled = EvalPrep(build_parser().parse_args(area + ["--tile", "208", "208"]), backend=backend, dataset=va).eval()
    assert tiled == plain
    doc = [(seeded_page(45, 150, 6, torch.float32)[None], [dict(label="ab", x_min=3, y_min=5, x_max=90, y_max=30)], "odd/page.png")]
    acc, cer = EvalPrep(build_parser().parse_args(base + ["--tile", "208", "208"]), backend=backend, dataset=doc).eval()
    assert 0.0 <= acc <= 1.0 and cer >= 0.0


def test_clean_cli_on_the_host_backend(tmp_path):
    """clean_cli.py with the oracle as the backend: PNGs of the same odd sizes and stems, mode L, the bytes of clean_pages(..., out="u8");
    two inputs with one stem are refused before anything is written."""
    from PIL import Image
    import clean_cli
    from oracle.modules import OracleCRNN, OracleUNet
    from qea.pages import clean_pages
    from qea.trainer_core import Backend
    backend = Backend(OracleUNet, OracleCRNN, torch.nn.CTCLoss, torch.optim.Adam, torch.device("cpu"), gpu_jitter=False)
    prep = OracleUNet(seed=5).eval()
    torch.save(prep, tmp_path / "prep")
    (tmp_path / "in").mkdir()
    g = torch.Generator().manual_seed(9)
    scans = {"a": torch.randint(0, 256, (21, 67), generator=g, dtype=torch.uint8), "b": torch.randint(0, 256, (35, 219), generator=g, dtype=torch.uint8)}
    Image.fromarray(scans["a"].numpy()).save(tmp_path / "in" / "a.png")
    Image.fromarray(scans["b"].numpy()).save(tmp_path / "in" / "b.PNG")
    args = clean_cli.build_parser().parse_args(["--prep_path", str(tmp_path / "prep"), "--in_dir", str(tmp_path / "in"),
                                                "--out_dir", str(tmp_path / "out"), "--tile", "208", "208", "--batch_pages", "1"])
    written = clean_cli.CleanPages(args, backend=backend).run()
    assert [p.split("/")[-1] for p in written] == ["a.png", "b.png"]
    want = clean_pages(prep, [scans["a"], scans["b"]], tile=(208, 208), out="u8")
    for path, w in zip(written, want):
        with Image.open(path) as img:
            assert img.mode == "L" and img.size == (w.shape[1], w.shape[0]) and np.array_equal(np.asarray(img), w.numpy())
    Image.fromarray(scans["a"].numpy()).save(tmp_path / "in" / "a.jpg")
    with pytest.raises(ValueError, match="stems"):
        clean_cli.CleanPages(args, backend=backend)


def test_library_exports_the_page_tile_entry_points():
    import ctypes as C
    from qea import _lib
    protos = {n: (r, a) for n, r, a in _lib.header_prototypes()}
    assert len(protos["qea_page_tiles_gather"][1]) == 14 and len(protos["qea_page_tiles_scatter"][1]) == 13
    L = _lib.lib()
    assert hasattr(L, "qea_page_tiles_gather") and hasattr(L, "qea_page_tiles_scatter") and L.qea_version() == 9
    one = C.c_void_p(256)                       # refused before any launch: nothing is dereferenced on the host
    assert L.qea_page_tiles_gather(None, 0, 1, None, None, None, 1, None, 1, 16, 16, None, None, None) < 0
    assert L.qea_page_tiles_gather(one, 0, 1, one, one, one, 1, one, 1, 16, 18, one, one, None) < 0         # TW no multiple of 4
    assert L.qea_page_tiles_gather(one, 0, 1, one, one, one, 1, one, 1, 16, 16, None, one, None) < 0        # 8-bit store, no table
    assert L.qea_page_tiles_gather(one, 2, 1, one, one, one, 1, one, 1, 16, 16, one, one, None) < 0         # unknown flag
    assert L.qea_page_tiles_gather(one, 0, 1, one, one, one, 1, one, 1, 16, 16, one, C.c_void_p(264), None) < 0   # out misaligned
    assert L.qea_page_tiles_scatter(one, 1, 16, 16, one, one, one, one, 1, 1, None, None, None) < 0         # no output at all
    assert L.qea_page_tiles_scatter(C.c_void_p(264), 1, 16, 16, one, one, one, one, 1, 1, one, None, None) < 0    # tiles misaligned
    assert L.qea_page_tiles_scatter(one, 1, 16, 16, one, one, one, one, 1, 0, one, None, None) < 0          # an empty store
    assert b"qea_page_tiles_scatter" in L.qea_last_error()


def test_clean_cli_and_eval_prep_flags():
    import clean_cli
    from qea.cli_flags import build_parser
    a = clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b", "--tile", "320", "336"])
    assert a.tile == [320, 336] and a.batch_pages == 8 and a.in_dir == "a" and a.out_dir == "b" and a.prep_path
    assert clean_cli.build_parser().parse_args(["--in_dir", "a", "--out_dir", "b"]).tile == [1024, 1024]
    v = build_parser("v", "")
    assert v.parse_args([]).tile is None and v.parse_args(["--tile", "320", "320"]).tile == [320, 320]
    for tag in "pacer":
        assert not hasattr(build_parser(tag, "").parse_args([] if tag != "r" else ["--cers_tess_path", "x"]), "tile")


def test_packed_store_helpers():
    """the Python side of a packed store (qea/pages.py): the size bounds each caller asks for, seen through .shape alone; open_store on the
    host; host_pages and pack_host as a round trip"""
    from types import SimpleNamespace
    from qea._lib import QeaError
    from qea.pages import (check_page_sizes, host_page, host_pages, is_int, open_store, pack_host, pack_ink_host, pack_pages, packed_result,
                           quantise_u8, require_eval)
    stub = lambda *shape: SimpleNamespace(shape=shape)          # nothing behind it: only .shape may be looked at
    ok, wide, huge, both = stub(400, 512), stub(2, 32768), stub(1 << 14, (1 << 13) + 1), stub(1, 40000, 4000)
    for bounds in (dict(), dict(max_pixels=1 << 27), dict(max_side=32767, max_pixels=1 << 27), dict(max_side=32767)):
        check_page_sizes([ok, stub(1, 1), stub(1, 32767, 4096), stub(7), object()], **bounds)
    check_page_sizes([wide], max_pixels=1 << 27)                # binarize and components: pixels only
    check_page_sizes([huge], max_side=32767)                    # reading: sides only
    check_page_sizes([wide, huge, both])                        # no bound at all
    for pages, bounds, words in (([ok, huge], dict(max_pixels=1 << 27), ["page 1", "16384 x 8193", "2^27"]),
                                 ([huge], dict(max_side=32767, max_pixels=1 << 27), ["page 0", "2^27"]),
                                 ([ok, ok, wide], dict(max_side=32767, max_pixels=1 << 27), ["page 2", "2 x 32768", "32767"]),
                                 ([wide], dict(max_side=32767), ["32767"]),
                                 ([both], dict(max_side=32767, max_pixels=1 << 27), ["40000 x 4000", "32767", "2^27"])):
        with pytest.raises(QeaError) as e:
            check_page_sizes(pages, **bounds)
        assert all(word in str(e.value) for word in words), (str(e.value), words)
    with pytest.raises(QeaError, match="32767"):
        check_page_sizes([wide], 32767, 1 << 27)                # the positional order deskew uses
    assert is_int(3) and is_int(np.int32(3)) and not is_int(True) and not is_int(3.0) and not is_int("3")

    g = torch.Generator().manual_seed(8)
    grey = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in ((3, 5), (1, 1), (4, 2))]
    real = [torch.rand(1, 3, 5, generator=g, dtype=torch.float64) * 1.5 - 0.25, torch.rand(2, 2, generator=g, dtype=torch.float64)]
    for pages in (grey, real):
        pk, dev, store, table = open_store(pages, None, 32767, 1 << 27)
        assert dev.type == "cpu" and store is pk.store and table is None and store.dtype == pages[0].dtype
        assert pk.offset.tolist() == np.concatenate([[0], np.cumsum([p.shape[-2] * p.shape[-1] for p in pages])[:-1]]).tolist()
        views = list(host_pages(pk))
        for p, (page, v) in enumerate(zip(pages, views)):
            assert v.dtype == np.uint8 and v.shape == tuple(page.shape[-2:]) and np.array_equal(v, host_page(pk, p))
            assert np.array_equal(v, (page if page.dtype == torch.uint8 else quantise_u8(page)).reshape(v.shape).numpy())
        back = pack_host(pk, views, torch.uint8)                # the round trip: the packed 8-bit form of the store
        assert back.dtype == torch.uint8 and torch.equal(back, store if store.dtype == torch.uint8 else quantise_u8(store))
        assert all(np.array_equal(a, b) for a, b in zip(host_pages(pk._replace(store=back)), views))
        labels = pack_host(pk, [np.arange(v.size, dtype=np.int64).reshape(v.shape).T.copy().T for v in views], torch.int32)   # strided arrays too
        assert labels.dtype == torch.int32 and labels.tolist() == [i for v in views for i in range(v.size)]
        for out, hi in (("u8", 255), ("float", 1.0)):
            ink = pack_ink_host(pk, [v <= 127 for v in views], out)
            assert ink.dtype == (torch.uint8 if out == "u8" else torch.float32)
            assert torch.equal(ink, torch.where(back <= 127, 0, hi).to(ink.dtype))
    assert open_store(grey, "cpu")[1] == torch.device("cpu")
    with pytest.raises(QeaError, match="2\\^27"):
        open_store([torch.zeros(1, dtype=torch.uint8).expand(1 << 14, (1 << 13) + 1)], None, max_pixels=1 << 27)     # refused before it is packed
    with pytest.raises(ValueError):
        open_store([])

    for out, dtype, key in (("u8", torch.uint8, "out_u8"), ("float", torch.float32, "out_f32")):
        res, kw = packed_result(6, out, torch.device("cpu"))
        assert res.dtype == dtype and res.shape == (6,) and list(kw) == [key] and kw[key] is res
    bn = torch.nn.Sequential(torch.nn.Conv2d(1, 1, 1), torch.nn.BatchNorm2d(1))
    require_eval(bn.eval(), "clean_pages")
    bn[1].train()
    for who in ("clean_pages", "read_pages"):
        with pytest.raises(ValueError, match=f"{who}.*eval"):
            require_eval(bn, who)
