"""CPU: the placement helpers of tests/hip_util.py (tests/test_train_placement_gpu.py and tests/test_disc_placement_gpu.py are only as
good as these), and the residues the project's trainers and discriminators give their flat-buffer views.

Plain torch stand-ins for a faulty kernel get what a kernel gets -- the views, as pointers: `_raw` reaches around a view the way an index
that is off by one does -- and each planted fault must be reported with the operand, the side and the element offset."""
import pytest
import torch

from tests.hip_util import (GUARD, PLACE_KINDS, assert_placement, discriminator_layouts, discriminator_residues, flat_buffer_offsets,
                            flat_buffer_residues, int_grid, place, trainer_residues)

N = 37                                  # not a multiple of 4: the views end inside a 16-byte granule


def _raw(view, first, count):
    """`count` elements from element `first` of the view's own allocation, relative to the view's first element."""
    return torch.as_strided(view, (count,), (1,), view.storage_offset() + first)


def _run(kernel, lead=GUARD, dtype=torch.float32):
    x, b = int_grid((N,), 1).to(dtype), int_grid((N,), 2).to(dtype)
    ins = place({"x": x, "b": b}, lead, "in")
    outs = place({"y": (N,), "aux": (5,)}, lead, "out", dtype=dtype)
    kernel(ins["x"], ins["b"], outs["y"])
    outs["aux"][:] = 1
    return ins, outs, x + b


def k_correct(x, b, y):
    y[:] = x + b


def k_store_before(x, b, y):
    y[:] = x + b
    _raw(y, -1, 1)[0] = 3.0


def k_store_past(x, b, y):
    y[:] = x + b
    _raw(y, N, 1)[0] = 3.0


def k_last_unwritten(x, b, y):
    y[:N - 1] = (x + b)[:N - 1]


def k_modifies_input(x, b, y):
    y[:] = x + b
    x[4] += 1


def k_masked_stray_load(x, b, y):
    """the last element's next tap lies past the input and is masked with a multiply: 0 * x[N]"""
    y[:] = x + b + 0 * _raw(x, 1, N)


@pytest.mark.parametrize("lead", [GUARD, GUARD + 1, GUARD + 2, GUARD + 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_a_correct_kernel_passes_at_every_residue(lead, dtype):
    ins, outs, ref = _run(k_correct, lead, dtype)
    assert_placement(ins, "inputs")
    assert_placement(outs, "outputs")
    assert torch.equal(outs["y"], ref)
    per16 = 16 // ref.element_size()
    for buf in (ins, outs):
        assert [buf.offset(n) % per16 for n in buf.names] == [lead % per16] * len(buf.names)
        assert buf.offset(buf.names[0]) == lead and all(v.is_contiguous() for v in buf)
        # every guard is at least GUARD wide, the last one included
        ends = [0] + [s + n for s, n in buf.spans]
        starts = [s for s, _ in buf.spans] + [buf.flat.numel()]
        assert all(s - e >= GUARD for e, s in zip(ends, starts))


@pytest.mark.parametrize("kernel,buf,needles", [
    (k_store_before, "outs", ("operand 'y'", "BEFORE", "element offset -1")),
    (k_store_past, "outs", ("operand 'y'", "PAST", f"element offset {N} ")),
    (k_last_unwritten, "outs", ("operand 'y'", "NEVER WRITTEN", f"element offset {N - 1} ")),
    (k_modifies_input, "ins", ("operand 'x'", "INPUT was modified", "element offset 4")),
    (k_masked_stray_load, "outs", ("operand 'y'", "NaN", "GUARD", f"element offset {N - 1}:")),
], ids=lambda v: v.__name__ if callable(v) else None)
def test_each_planted_fault_is_named(kernel, buf, needles):
    ins, outs, _ = _run(kernel)
    bufs = {"ins": ins, "outs": outs}
    with pytest.raises(AssertionError) as e:
        assert_placement(bufs[buf], "case 7")
    s = str(e.value)
    assert s.startswith("case 7: ") and all(n in s for n in needles), s
    assert s.count("operand '") == 1, s                      # ... and nothing else is blamed
    assert_placement(bufs["ins" if buf == "outs" else "outs"], "the other buffer")


def test_a_stray_store_is_blamed_on_the_nearer_operand():
    outs = place({"a": (8,), "b": (8,)}, GUARD + 2, "out")
    for v in outs:
        v[:] = 0
    between = outs.offset("a") + 8
    outs.flat[between + 2] = 1.0                            # 3 past a, far before b
    with pytest.raises(AssertionError, match=r"operand 'a': a store PAST the view, at element offset 10 \(size 8\)"):
        assert_placement(outs)
    outs.flat[between + 2] = outs.flat[between + 3]         # (the guard's own pattern back)
    assert_placement(outs)
    outs.flat[outs.offset("b") - 2] = 1.0
    with pytest.raises(AssertionError, match=r"operand 'b': a store BEFORE the view, at element offset -2"):
        assert_placement(outs)


def test_accumulating_outputs_keep_their_prefill_and_show_a_consumed_guard():
    pre = int_grid((6, 3), 5, -100, 100)
    acc = place({"dw": pre, "total": torch.zeros(3)}, GUARD + 2, "acc")
    acc["dw"].add_(2)
    assert_placement(acc)
    assert torch.equal(acc["dw"], pre + 2) and acc["dw"].shape == (6, 3)
    x = place({"x": torch.ones(3)}, GUARD, "in")
    acc["total"].add_(_raw(x["x"], 1, 3) * 0)
    with pytest.raises(AssertionError, match=r"operand 'total': 1 accumulated elements are NaN, first at element offset 2"):
        assert_placement(acc)


def test_guards_and_prefills_are_what_the_docstring_says():
    i, o = place({"x": torch.zeros(3)}, GUARD, "in"), place({"y": (3,)}, GUARD, "out")
    assert bool(torch.isnan(i.flat[:GUARD]).all()) and bool(torch.isnan(o["y"]).all())
    g = o.flat[:GUARD]
    assert bool(torch.isfinite(g).all()) and float(g.abs().min()) > 1e30      # no result of a test comes near it
    # the two NaN patterns differ: a never-written element and a consumed guard are told apart bit for bit
    assert not torch.equal(i.flat[:1].view(torch.int32), o["y"][:1].view(torch.int32))
    with pytest.raises(AssertionError):
        place({"x": torch.zeros(3)}, GUARD - 1, "in")
    with pytest.raises(AssertionError):
        place({"x": (3,)}, GUARD, "in")                     # an input needs values


def test_the_gpu_tests_run_the_residues_the_trainers_produce():
    """offset % 4 of every parameter / gradient view of VAEDecoderTrainer, VAETrainer and UNetTrainer (full and nuScenes), from the
    shape tables and orders those trainers use.  The shipped VAE's 2-float `decoder.conv_out.bias` would put whatever follows it at
    residue 2 -- but the decoder is last in both VAE trainers' order and conv_out is last in the decoder, so nothing follows it: every
    view of these three tape trainers starts on a 16-byte boundary today.  (Of these three only: the discriminators keep flat buffers
    too, and the Meta-Kernel network's do not -- test_the_discriminators_residues below.)  tests/test_train_placement_gpu.py takes its
    list from the same function, so it follows a configuration that changes the set."""
    from tests import test_train_placement_gpu as G
    per = trainer_residues()
    assert set(per) == {f"{t}/{p}" for t in ("VAEDecoderTrainer", "VAETrainer", "UNetTrainer") for p in ("RangeLDM", "nuscenes")}
    derived = set().union(*per.values())
    assert list(G.RESIDUES) == sorted(derived)
    assert derived == {0}, per
    # the derivation itself: a 2-float parameter in the middle moves what follows it
    shapes = {"a.weight": (2, 64, 3, 3), "a.bias": (2,), "b.weight": (8, 2), "b.bias": (3,), "c.bias": (4,)}
    assert flat_buffer_residues(list(shapes), shapes) == {0, 2, 1}
    from rangeldm_amd.config import PRESETS
    from rangeldm_amd.params import vae_param_shapes
    from rangeldm_amd.vae_training import decoder_param_names
    vs = vae_param_shapes(PRESETS["RangeLDM"]["vae"])
    names = decoder_param_names(PRESETS["RangeLDM"]["vae"], vs)
    assert names[-1] == "decoder.conv_out.bias" and tuple(vs[names[-1]]) == (2,)


def test_the_discriminators_residues():
    """offset % 4 of every parameter / gradient view of PatchDiscriminator and MetaKernelDiscriminator (hip_util.discriminator_layouts:
    the image and disc_bev PatchGANs, the Meta-Kernel network at its default and at the tests' configs).  Every PatchGAN parameter is a
    multiple of 16 floats but the last bias, which nothing follows: {0}.  The Meta-Kernel network's first layer has C = 2 --
    mlp_coord.0.weight 6 floats, mlp_coord.0.bias 2, mlp_coord.2.weight 4, mlp_coord.2.bias 2: 14 floats in front of coov.weight -- and
    every later parameter is a multiple of 4 floats, so the 8-byte offset stays to the end of the buffer: {0, 2}.
    tests/test_disc_placement_gpu.py takes its list from the same function."""
    from tests import test_disc_placement_gpu as G
    per = discriminator_residues()
    layouts = discriminator_layouts()
    assert set(per) == set(layouts) and len(per) >= 8
    patch = {k for k in per if k.startswith("PatchDiscriminator/")}
    meta = {k for k in per if k.startswith("MetaKernelDiscriminator/")}
    assert patch and meta and patch | meta == set(per)
    assert {"PatchDiscriminator/image", "PatchDiscriminator/disc_bev/gz16", "MetaKernelDiscriminator/default"} <= set(per)
    for k in patch:
        assert per[k] == {0}, (k, per[k])
    for k in meta:
        assert per[k] == {0, 2}, (k, per[k])
        names, shapes = layouts[k]
        off = flat_buffer_offsets(names, shapes)
        assert set(off.values()) == per[k] and list(off) == list(names)
        at2 = [n for n in names if off[n] == 2]
        assert at2[0] == "main.0.mlp_coord.0.bias"
        tail = names[names.index("main.0.coov.weight"):]
        assert all(off[n] == 2 for n in tail), [n for n in tail if off[n] != 2]
        assert [n for n in names if off[n] == 0] == ["main.0.mlp_coord.0.weight", "main.0.mlp_coord.2.weight", "main.0.mlp_coord.2.bias"]
        # ... which is every later MLP weight, every coov weight and bias, every BatchNorm gamma and beta
        assert any(n.endswith(".mlp_coord.2.weight") for n in tail) and any(n.endswith("coov.bias") for n in tail)
        assert any(n.startswith("main.3.") for n in tail)
    assert list(G.DISC_RESIDUES) == sorted(set().union(*per.values())) == [0, 2]


# ---- kind "scratch": a caller-owned workspace ------------------------------------------------------------------------------------------
def _scratch(kernel, lead=GUARD, dtype=torch.float32):
    ws = place({"ws": (N,), "partials": (6,)}, lead, "scratch", dtype=dtype)
    kernel(ws["ws"])
    return ws


def k_ws_untouched(ws):
    pass


def k_ws_partly_written(ws):
    ws[:N // 2] = 1.5


def k_ws_holds_foreign_nans(ws):
    """the low words of fp64 partials seen through an fp32 view, the unwritten pattern next to them"""
    ws[3] = float("nan")
    ws[4:8] = torch.tensor([1.0, -2.5], dtype=torch.float64).view(ws.dtype)[:4] if ws.dtype == torch.float32 else 0.0


def k_ws_store_past(ws):
    ws[:] = 0
    _raw(ws, N, 1)[0] = 3.0


def k_ws_store_before(ws):
    ws[:] = 0
    _raw(ws, -2, 1)[0] = 3.0


def test_scratch_is_a_fourth_kind_and_changes_no_other():
    assert PLACE_KINDS == ("in", "out", "acc", "scratch")
    ws, o = place({"ws": (5,)}, GUARD + 2, "scratch"), place({"ws": (5,)}, GUARD + 2, "out")
    assert torch.equal(ws.flat.view(torch.int32), o.flat.view(torch.int32))           # an output's sentinels and unwritten pattern
    assert ws.kind == "scratch" and ws["ws"].shape == (5,) and ws.offset("ws") % 4 == 2
    with pytest.raises(AssertionError):
        place({"ws": (5,)}, GUARD, "workspace")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kernel", [k_ws_untouched, k_ws_partly_written, k_ws_holds_foreign_nans], ids=lambda k: k.__name__)
def test_scratch_interior_is_not_judged(kernel, dtype):
    """A workspace may stay unwritten, be written in part, or hold any bit pattern: only the guards are checked -- where the same
    interior fails as an "out"."""
    assert_placement(_scratch(kernel, GUARD + 2, dtype), "workspace")
    out = place({"ws": (N,)}, GUARD, "out", dtype=dtype)
    kernel(out["ws"])
    with pytest.raises(AssertionError, match="NEVER WRITTEN"):
        assert_placement(out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kernel,needles", [
    (k_ws_store_past, ("operand 'ws'", "PAST", f"element offset {N} ")),
    (k_ws_store_before, ("operand 'ws'", "BEFORE", "element offset -2")),
], ids=lambda v: v.__name__ if callable(v) else None)
def test_a_store_outside_a_scratch_view_is_named(kernel, needles, dtype):
    ws = _scratch(kernel, GUARD, dtype)
    with pytest.raises(AssertionError) as e:
        assert_placement(ws, "case 9")
    s = str(e.value)
    assert s.startswith("case 9: ") and all(n in s for n in needles), s
    assert s.count("operand '") == 1, s
