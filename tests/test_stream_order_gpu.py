"""What runs on two streams, under a delayed stream (tests/stream_stress.py): the engines' backward with every weight gradient held
back until the main chain has run to its end, the abs-max pool when it runs out of slots, and the three host-to-device staging sites
with their copies held back while the host goes on.  Every comparison is exact: the side stream runs its work in the single-stream
order, and the wgrad and one-channel kernels use no atomics.

The teeth tests show on a dummy owner that the window is really open: each broken rule of SideStream.run gives the stale value it
must give, and the protected form of the same lines the right one."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

import helpers as H
import resident_docs_fixture as DF
import resident_fixture as RF
import stream_stress as SS

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
try:
    import engine_schedule as E
finally:
    sys.path.pop(0)

GRAD_CASES = [c for c, v in E.CASES.items() if v[3]]
assert len(GRAD_CASES) == 10
N2MB = (2 << 20) // 4                       # fp32 elements of a 2 MB tensor


class _Owner:
    pass


# ----------------------------------------------------------------------------- the engines
def _engine_pass(case, seed, delay_ms=None):
    """One forward + backward of `case` as tools/engine_schedule._run builds it -> ({name: tensor}, the Window or None).
    delay_ms: the backward alone runs under delayed_side."""
    from oracle import model_oracle as mo
    kind, B, train, grad, kwargs, _ = E.CASES[case]
    x = H.synth_images(B, seed).cuda()
    if kind == "unet":
        from models.model_unet import UNet
        net = UNet()
        net.load_state_dict(mo.seeded_state(mo.unet_state_shapes(), seed + 1))
        net = net.cuda().train(train)
    else:
        from models.model_crnn import CRNN
        net = CRNN(95, False)
        net.load_state_dict(mo.seeded_state(mo.crnn_state_shapes(), seed + 1))
        net = net.cuda().train()
        net.register_backward_hook(net.backward_hook)
        if not train:
            for m in net.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.eval()
        x.requires_grad_()
    out = net(x, **kwargs)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed + 2)).cuda()
    win = None
    if delay_ms is None:
        out.backward(dout)
    else:
        with SS.delayed_side(net._qea_engine, delay_ms) as win:
            out.backward(dout)
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    if x.grad is not None:
        res["dx"] = x.grad
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        res["G:" + n] = p.grad
    for n, b in net.named_buffers():
        res["B:" + n] = b
    return {k: v.clone() for k, v in res.items()}, win


@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("case", GRAD_CASES)
def test_backward_with_the_side_stream_held_back(case, mode):
    """Every case of tools/engine_schedule.py that takes a gradient, in both MFMA modes: the backward with all side-stream work pending
    behind the spin until the main chain has finished on the device (so that every buffer the main chain frees has been handed out
    again, and every in-place write done, before the first weight gradient reads anything) gives bit for bit the output, input
    gradient, parameter gradients and buffers of the same pass on one stream."""
    from qea import crnn_engine, ops, unet_engine
    engine = unet_engine if E.CASES[case][0] == "unet" else crnn_engine
    off = E.CASES[case][5]
    seed = 300 + 10 * list(E.CASES).index(case)
    before = {name: getattr(engine, name) for name in off}
    prev_mode, prev_overlap = ops.set_mfma_mode(mode), ops.overlap_enabled()
    try:
        for name in off:
            setattr(engine, name, False)
        ops.set_overlap(False)
        want, _ = _engine_pass(case, seed)
        ops.set_overlap(True)
        got, win = _engine_pass(case, seed, SS.D_MS)
    finally:
        ops.set_overlap(prev_overlap)
        ops.set_mfma_mode(prev_mode)
        for name, v in before.items():
            setattr(engine, name, v)
    print(f"\nchain {case}/{mode}: {win.chain_ms:.1f} ms from the spin's enqueue to the drained main stream (spin {SS.D_MS} ms, "
          f"on {'its own' if win.own_stream else 'a substituted'} side stream)")
    assert win.checks == 1 and sorted(got) == sorted(want)
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, f"{len(bad)} of {len(want)} tensors differ from the single-stream pass: {bad[:8]}"


# ----------------------------------------------------------------------------- teeth: the window is open
@pytest.mark.parametrize("listed", [False, True])
def test_teeth_reuse_of_a_freed_read(listed):
    """Rule (a).  fn copies t; the main stream frees t and allocates the same size.  Not listed in `reads`: the allocator hands t's
    memory out again and the copy holds what the main stream wrote there.  Listed: another block, and the copy holds t."""
    from qea import ops
    owner, box, got = _Owner(), [], []
    gc.collect()
    with SS.delayed_side(owner, SS.D_MS):
        side = ops.SideStream.of(owner, torch.device("cuda", torch.cuda.current_device()))
        t = torch.empty(N2MB, device="cuda").fill_(1)
        box.append(t)
        side.run(lambda: got.append(torch.empty_like(box[0]).copy_(box[0])), *([t] if listed else []))
        old = t.data_ptr()
        box.clear()
        del t
        u = torch.empty(N2MB, device="cuda").fill_(7)
        side.join()
    torch.cuda.synchronize()
    if listed:
        assert u.data_ptr() != old, "a tensor recorded on the side stream was handed out again while its reader was pending"
        assert bool((got[0] == 1).all())
    else:
        assert u.data_ptr() == old, "allocator did not reuse; the probe proves nothing"
        assert bool((got[0] == 7).all())


def test_teeth_in_place_write_under_a_pending_read():
    """Rule (b).  fn reads t, the main stream then zeroes t in place: the copy holds 0 although t is listed in `reads` (record_stream
    protects the memory, not the values).  The protected form zeroes a buffer of its own."""
    from qea import ops
    owner, got = _Owner(), []
    with SS.delayed_side(owner, SS.D_MS):
        side = ops.SideStream.of(owner, torch.device("cuda", torch.cuda.current_device()))
        t, t2 = torch.empty(N2MB, device="cuda").fill_(1), torch.empty(N2MB, device="cuda").fill_(1)
        side.run(lambda: got.append(torch.empty_like(t).copy_(t)), t)
        t.zero_()
        side.run(lambda: got.append(torch.empty_like(t2).copy_(t2)), t2)
        z = torch.zeros_like(t2)                                     # the zeros go to a buffer of the main stream's own
        side.join()
    torch.cuda.synchronize()
    assert bool((got[0] == 0).all()) and bool((got[1] == 1).all()) and bool((z == 0).all())


def test_teeth_read_before_the_join():
    """Rule (c).  fn writes g; a copy the main stream takes before join() holds the old values, one taken after it the new ones."""
    from qea import ops
    owner = _Owner()
    with SS.delayed_side(owner, SS.D_MS):
        side = ops.SideStream.of(owner, torch.device("cuda", torch.cuda.current_device()))
        g = torch.empty(N2MB, device="cuda").fill_(1)
        side.run(lambda: g.fill_(5), g)
        early = g.clone()
        side.join()
        late = g.clone()
    torch.cuda.synchronize()
    assert bool((early == 1).all()) and bool((late == 5).all())


# ----------------------------------------------------------------------------- the abs-max pool
def test_amax_pool_keeps_a_full_buffer_for_pending_readers():
    """AmaxPool starts a new buffer when its slots run out.  The engines hold slots in locals and do not list them in `reads`, so a
    pending side-stream reader of an old slot depends on the POOL keeping the old buffer: dropped, its 512-byte block goes back to
    the allocator and the next small tensors of the main stream land on it."""
    from qea import ops
    owner, box, got = _Owner(), [], []
    gc.collect()
    pool = ops.AmaxPool(torch.device("cuda", torch.cuda.current_device()), n=2)
    s0, s1 = pool(), pool()
    s1.fill_(3.0)
    with SS.delayed_side(owner, SS.D_MS):
        side = ops.SideStream.of(owner, torch.device("cuda", torch.cuda.current_device()))
        box.append(s1)
        side.run(lambda: got.append(box[0].clone()))
        s2, s3 = pool(), pool()
        assert s2.data_ptr() != s0.data_ptr() and s3.data_ptr() == s2.data_ptr() + 4 and pool.used == 2       # a new buffer, slots 0 and 1
        box.clear()
        del s0, s1
        later = [torch.empty(2, device="cuda").fill_(99) for _ in range(16)]
        side.join()
    torch.cuda.synchronize()
    assert got[0].item() == 3.0, f"the side stream read {got[0].item()} from slot 1 of the full buffer, the main stream wrote 3.0 there"
    assert len(later) == 16


# ----------------------------------------------------------------------------- staging
def _history(seed, n, W):
    labels = H.synth_labels(n * (W + 1), seed, lo=1, hi=9)
    names = [f"img{i}" for i in range(n)]
    return {name: labels[i * (W + 1):(i + 1) * (W + 1)] for i, name in enumerate(names)}, names


@pytest.mark.parametrize("kind", ["levenshtein", "attention"])
def test_label_packer_reuses_its_pinned_buffer_after_the_copy(kind):
    """pack/to_device of data A with the copy held back, then at once pack/to_device of data B of the same size into the same pinned
    buffer: the first device tensor holds A (the second pack waits for the first copy: bounded by the spin), the second B."""
    from qea import history
    W, n = 4, 12
    pk = history.LevenshteinPacker(W) if kind == "levenshtein" else history.AttentionPacker(W, H.C2I)
    (hist_a, names), (hist_b, _) = _history(1, n, W), _history(2, n, W)
    warm = pk.to_device(pk.pack(hist_b, names), "cuda")               # the pinned buffer and both label sets' rows exist
    torch.cuda.synchronize()
    with SS.delayed_current(SS.D_MS) as win:
        packed_a = pk.pack(hist_a, names)
        dev_a = pk.to_device(packed_a, "cuda")
        host_a = np.array(packed_a[0], copy=True)
        win.require_open("LabelPacker.to_device")
        packed_b = pk.pack(hist_b, names)
        assert packed_b[1].data_ptr() == packed_a[1].data_ptr() and len(packed_b[0]) == len(host_a)
        dev_b = pk.to_device(packed_b, "cuda")
        host_b = np.array(packed_b[0], copy=True)
    assert not np.array_equal(host_a, host_b)
    assert np.array_equal(dev_a.cpu().numpy(), host_a) and np.array_equal(dev_b.cpu().numpy(), host_b)
    assert np.array_equal(warm.cpu().numpy(), host_b)


def test_strip_store_batches_with_the_copies_held_back(tmp_path):
    """_PackedStore._batch frees its pinned index block right after a non-blocking copy: two batches in a row with the copies held
    back equal the same calls made with nothing in the way."""
    from datasets.img_dataset import ImgDataset
    from datasets.resident import ResidentStrips
    RF.write_strips(str(tmp_path))
    dev = ResidentStrips(ImgDataset(str(tmp_path), transform=RF.pad_transform(), include_name=True), RF.SIZE, device="cuda")
    rows_a, rows_b = [0, 5, 9, 17, 23], [22, 3, 3, 11, 8]
    want_a, want_b = dev.batch(rows_a).clone(), dev.batch(rows_b).clone()
    torch.cuda.synchronize()
    assert not torch.equal(want_a, want_b)
    with SS.delayed_current(SS.D_MS) as win:
        got_a = dev.batch(rows_a)
        got_b = dev.batch(rows_b)
        win.require_open("ResidentStrips.batch")
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)


def test_document_crops_with_the_copies_held_back(tmp_path):
    """ResidentDocuments.crops, the same way: its (doc, strip_first) block is pinned, copied without waiting and freed at once."""
    from datasets.patch_dataset import PatchDataset
    from datasets.resident import ResidentDocuments
    dev = ResidentDocuments(PatchDataset(DF.write_documents(str(tmp_path)), pad=True, include_name=True), device="cuda")
    rows_a, rows_b = [DF.ONE, DF.OVERLAP, DF.WIDE], [DF.TALL, DF.PLACEHOLDER, DF.CORNERS]
    x = torch.rand(3, 1, *DF.CANVAS, generator=torch.Generator().manual_seed(21)).cuda()
    want_a, want_b = dev.crops(x, rows_a, 32, 128).clone(), dev.crops(x, rows_b, 32, 128).clone()
    want_d = dev.batch(rows_a).clone()
    torch.cuda.synchronize()
    assert want_a.shape[0] == 9 and want_b.shape[0] == 40
    with SS.delayed_current(SS.D_MS) as win:
        got_a = dev.crops(x, rows_a, 32, 128)
        got_b = dev.crops(x, rows_b, 32, 128)
        got_d = dev.batch(rows_a)
        win.require_open("ResidentDocuments.crops")
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b) and torch.equal(got_d, want_d)
