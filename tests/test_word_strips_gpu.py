"""Word strips and read_pages on the MI355X (csrc/word_strips.hip): the kernel bit for bit the statement tests/word_strips_spec.py over a
ragged store with junk between the pages, the device path against the host path and against utils.get_text_stack where nothing is
resampled, read_pages against utils.pred_to_string on the very score tensors its passes produced, the front end, and the refusals of
the C ABI."""
import json

import numpy as np
import pytest
import torch

import word_strips_spec as spec
from test_word_strips_cpu import WIDTHS, boxes_for, cli_args, float_pages, pages_of, statement, tensors, u8_pages, word_scans

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _store(kind, seed=5):
    """the three pages in ONE store with junk between them, every page at an odd element offset, the last page ending with the store, and
    the store itself starting three elements into its allocation -> (store on the device, offset, h, w)"""
    g = torch.Generator().manual_seed(seed)
    pages = pages_of(kind)
    offset, off = [], 1
    for px in pages:
        off += 1 - off % 2
        offset.append(off)
        off += px.size + 2
    off -= 2
    whole = torch.randint(0, 256, (off + 3,), generator=g, dtype=torch.uint8) if kind == "u8" else torch.rand(off + 3, generator=g) * 1.5 - 0.25
    for o, px in zip(offset, pages):
        whole[3 + o:3 + o + px.size] = torch.from_numpy(px.reshape(-1))
    store = whole.cuda()[3:]
    return store, np.asarray(offset, np.int64), np.asarray([p.shape[0] for p in pages], np.int32), np.asarray([p.shape[1] for p in pages], np.int32)


def _launches(before):
    from qea import ops
    return {k: ops.WORD_STRIP_LAUNCHES[k] - before[k] for k in before}


@pytest.mark.parametrize("OW", WIDTHS)
@pytest.mark.parametrize("kind", ["u8", "float"])
def test_the_kernel_is_the_statement_bit_for_bit(kind, OW):
    """every box of the issue, the 2049-row ones among them (the only place where 32-bit arithmetic would be wrong), in one launch that
    writes every element of out"""
    from qea import ops
    store, offset, h, w = _store(kind)
    assert store.data_ptr() % 16 != 0 and store.is_contiguous()
    table = ops.page_table(offset, h, w, store.device)
    boxes = torch.from_numpy(boxes_for(OW)).cuda()
    out = torch.full((len(boxes), 1, 32, OW), SENTINEL, device="cuda")
    before = dict(ops.WORD_STRIP_LAUNCHES)
    got = ops.word_strips(store, table, boxes, OW, torch.from_numpy(spec.norm()).cuda(), out=out)
    assert _launches(before) == {"strips": 1} and got is out
    got, want = out.cpu().numpy(), statement(kind, OW)
    for i, b in enumerate(boxes_for(OW)):
        assert np.array_equal(got[i], want[i]), (i, b.tolist())
    assert 2049 in {min(int(b[4]), 2100) - max(int(b[2]), 0) for b in boxes_for(OW) if b[0] == 2}


@pytest.mark.parametrize("kind", ["u8", "float"])
def test_the_device_path_is_the_host_path(kind):
    from qea import ops
    from qea.reading import word_strips
    pages = tensors(kind)
    if kind == "float":
        pages = [p[None] if i % 2 else p for i, p in enumerate(pages)]
    for OW in WIDTHS + (512,):
        boxes = boxes_for(min(OW, 128))
        want = word_strips(pages, boxes, OW)
        before = dict(ops.WORD_STRIP_LAUNCHES)
        got = word_strips([p.cuda() for p in pages], boxes, OW)
        also = word_strips(pages, torch.from_numpy(boxes), OW, device="cuda")
        assert _launches(before) == {"strips": 2}
        assert got.is_cuda and also.is_cuda and got.dtype == torch.float32 and torch.equal(got.cpu(), want) and torch.equal(also.cpu(), want)
    assert tuple(word_strips([p.cuda() for p in pages], [], 64).shape) == (0, 1, 32, 64)


@pytest.mark.parametrize("OW", WIDTHS)
def test_boxes_of_at_most_32_rows_are_get_text_stack_on_the_device(OW):
    """the crop kernel of utils.get_text_stack and this one write identical strips where nothing is resampled"""
    from qea.reading import word_strips
    from utils import get_text_stack
    boxes = boxes_for(OW)
    got = word_strips([p.cuda() for p in tensors("u8")], boxes, OW)
    seen = 0
    for p, page in enumerate(u8_pages()):
        rows = [i for i, b in enumerate(boxes.tolist()) if b[0] == p and min(b[4], page.shape[0]) - max(b[2], 0) <= 32]
        if not rows:
            continue
        image = torch.from_numpy(spec.norm()[page])[None].cuda()
        labels = [dict(zip(("x_min", "y_min", "x_max", "y_max"), (max(v, 0) for v in boxes[i, 1:].tolist())), label="") for i in rows]
        want, _ = get_text_stack(image, labels, (32, OW))
        assert want.is_cuda and torch.equal(got[rows], want), p
        seen += len(rows)
    assert seen >= 14


def _crnn(seed=6):
    from models.model_crnn import CRNN
    from oracle import model_oracle as mo
    net = CRNN(95, False)
    net.load_state_dict(mo.default_init_state(mo.crnn_state_shapes(), seed))
    return net.cuda().eval()


@pytest.mark.parametrize("beam", [0, 4])
def test_read_pages_is_pred_to_string_of_its_own_passes(tmp_path, beam):
    """three small pages, default-init CRNN weights: a recording forward keeps every pass's scores; the strings (and scores) returned are
    pred_to_string of exactly those tensors scattered back into box order, and the passes are those of strip_plan: order and plumbing,
    without assuming that two runs of the CRNN agree bit for bit"""
    import properties
    from qea import ops
    from qea.components import word_boxes
    from qea.reading import box_table, read_pages, strip_plan, word_strips
    from utils import get_char_maps, pred_to_string
    scans = word_scans(tmp_path / "in")
    pages = [torch.from_numpy(px).cuda() for px in scans.values()]
    boxes = word_boxes(pages, gap_x=2, min_area=16)
    assert [len(b) for b in boxes] == [4, 2, 1]
    index_to_char = get_char_maps(properties.char_set)[1]
    model, seen = _crnn(), []

    def forward(x):
        s = model(x)
        seen.append((x.clone(), s.clone()))
        return s
    before = dict(ops.WORD_STRIP_LAUNCHES)
    res = read_pages(model, pages, boxes, index_to_char, buckets=(64, 128), strip_pixels=256, beam=beam, forward=forward)
    table = box_table(boxes)
    plan = strip_plan(table, [p.shape[0] for p in pages], [p.shape[1] for p in pages], (64, 128), 256)
    assert _launches(before) == {"strips": len({OW for OW, _ in plan.passes})} == {"strips": 2}
    assert [(x.shape[3], x.shape[0]) for x, _ in seen] == [(OW, len(idx)) for OW, idx in plan.passes] and len(seen) == 3
    texts, scores = [None] * len(table), [None] * len(table)
    for (x, s), (OW, idx) in zip(seen, plan.passes):
        assert x.is_cuda and torch.equal(x, word_strips(pages, table[idx], OW))
        if beam:
            t, v = pred_to_string(s, [""] * len(idx), index_to_char, beam=beam, return_scores=True)
        else:
            t, v = pred_to_string(s, [""] * len(idx), index_to_char), [None] * len(idx)
        for i, a, b in zip(idx.tolist(), t, v):
            texts[i], scores[i] = a, b
    split = lambda v: [v[0:4], v[4:6], v[6:7]]
    assert res[0] == split(texts) and res[-1] == 1 == int(plan.cut.sum())
    if beam:
        assert len(res) == 3 and res[1] == split(scores) and all(isinstance(s, float) for s in scores)
    else:
        assert len(res) == 2
    with pytest.raises(ValueError, match="eval"):
        read_pages(model.train(), pages, boxes, index_to_char)


def test_clean_cli_read_on_the_device(tmp_path, capsys):
    """--read on the device: every box of the JSON has a label (and a score with a beam), the boxes and the PNG bytes are those of the run
    without the flag"""
    import clean_cli
    word_scans(tmp_path / "in")
    torch.save(_crnn(), tmp_path / "crnn")
    plain = clean_cli.CleanPages(cli_args(tmp_path, "plain", "--boxes")).run()
    assert "words read" not in capsys.readouterr().out
    read = clean_cli.CleanPages(cli_args(tmp_path, "read", "--read", str(tmp_path / "crnn"), "--read_buckets", "64", "128")).run()
    printed = capsys.readouterr().out
    beam = clean_cli.CleanPages(cli_args(tmp_path, "beam", "--read", str(tmp_path / "crnn"), "--read_buckets", "64", "128", "--read_beam", "4")).run()
    assert len(plain) == len(read) == len(beam) == 3
    for stem, count, p, r, b in zip("abc", (4, 2, 1), plain, read, beam):
        with open(p, "rb") as x, open(r, "rb") as y, open(b, "rb") as z:
            assert x.read() == y.read() == z.read()
        with open(p[:-4] + ".json") as x, open(r[:-4] + ".json") as y, open(b[:-4] + ".json") as z:
            want, got, scored = json.load(x), json.load(y), json.load(z)
        assert len(want) == count and all(row["label"] == "" for row in want)
        assert [dict(row, label="") for row in got] == want and all(isinstance(row["label"], str) for row in got)
        assert [dict(label="", **{k: row[k] for k in ("x_min", "y_min", "x_max", "y_max")}) for row in scored] == want
        assert all(isinstance(row["label"], str) and isinstance(row["score"], float) and row["score"] <= 0 for row in scored)
        assert f"{stem}: {count} words read, {int(stem == 'b')} cut\n" in printed


def test_library_refusals_launch_nothing():
    """the C ABI with real device buffers: every refusal returns a negative code and leaves the prefilled output untouched; the accepted
    call then writes all of it"""
    from qea import _lib, ops
    L = _lib.lib()
    page = u8_pages()[1]
    store = torch.from_numpy(page.reshape(-1).copy()).cuda()
    table = ops.page_table(np.zeros(1, np.int64), np.asarray([45], np.int32), np.asarray([67], np.int32), store.device)
    host_boxes = np.asarray([(0, 0, 0, 67, 45), (0, 5, 7, 60, 39)], np.int32)
    boxes = torch.from_numpy(host_boxes).cuda()
    norm = torch.from_numpy(spec.norm()).cuda()
    out = torch.full((2, 1, 32, 64), SENTINEL, device="cuda")

    def call(st=store.data_ptr(), f32=0, elems=store.numel(), offset=table.offset, h=table.h, w=table.w, n_pages=1, bx=boxes.data_ptr(), n=2, OW=64,
             nm=norm.data_ptr(), o=out.data_ptr()):
        return L.qea_word_strips(st, f32, elems, offset, h, w, n_pages, bx, n, OW, nm, o, None)
    for kw in (dict(OW=72), dict(OW=60), dict(OW=48), dict(OW=528), dict(OW=0), dict(OW=-64), dict(n=-1), dict(n=(1 << 20) + 1), dict(st=None),
               dict(offset=None), dict(h=None), dict(w=None), dict(bx=None), dict(nm=None), dict(o=None), dict(o=out.data_ptr() + 4), dict(f32=2),
               dict(st=store.data_ptr() + 1, f32=1), dict(elems=0), dict(n_pages=0)):
        assert call(**kw) < 0, kw
        assert b"qea_word_strips" in L.qea_last_error(), kw
    before = dict(ops.WORD_STRIP_LAUNCHES)
    for OW in (72, 48, 528):
        with pytest.raises(_lib.QeaError):
            ops.word_strips(store, table, boxes, OW, norm)
    with pytest.raises(_lib.QeaError):
        ops.word_strips(store, table, boxes, 64, norm, out=torch.empty(2, 1, 32, 128, device="cuda"))
    with pytest.raises(_lib.QeaError):
        ops.word_strips(store, table, boxes[:, :4].contiguous(), 64, norm)
    assert _launches(before) == {"strips": 0}
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), spec.strips([page], host_boxes, 64))
