"""CPU: the placement helpers of tests/hip_util.py (tests/test_train_placement_gpu.py is only as good as these), and the residues the
project's trainers give their flat-buffer views.

Plain torch stand-ins for a faulty kernel get what a kernel gets -- the views, as pointers: `_raw` reaches around a view the way an index
that is off by one does -- and each planted fault must be reported with the operand, the side and the element offset."""
import pytest
import torch

from tests.hip_util import GUARD, assert_placement, flat_buffer_residues, int_grid, place, trainer_residues

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
    view starts on a 16-byte boundary today.  The GPU test takes its list from the same function, so it follows a configuration that
    changes the set."""
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
