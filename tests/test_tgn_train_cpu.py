"""Base-TGN training (learn_base.py for --base_type tgn) on the CPU: the reference-shaped torch formulation of the
stateful step (tests/tgn_train_ref.py) against the reference's own four steps (tests/golden/tgn_train.npz) in fp32
and fp64, the closed-form backward the kernel tests use (with the gradient of a gathered node table) against
autograd, the C ABI of the HIP training pair, the model's and the memory's interface, and learn_base's switch.

Tolerances.  The fp32 formulation runs the reference's own operations in the reference's order on the same CPU
kernels: where the goldens were made its logits, loss, memory and stored raw messages are at 0 distance.  A GEMM's
blocking changes with the thread count, though, so these are asserted within tests/test_graphmixer_oracle.py's
ATOL / RTOL (5e-6 / 1e-5, the project's bound for an fp32 restatement of the same operations); last_update, the
timestamps and the set of nodes with a pending message are asserted equal.  Gradients
accumulate in another order (the formulation sums over a table, the reference over per-hop gathers), so per tensor
||g - g_ref32|| <= max(1e-5 ||g_ref32||, 3 ||g_ref32 - g_ref64||): tests/test_tgat_train_cpu.py's 1e-5 relative norm
for a stored fp32 gradient (measured here: 3.4e-6 at the thread count the goldens were made with, 2.5e-6 single
threaded), or, for a tensor whose reference fp32 error is larger than that, that error once for each of the two
fp32 runs and once over.  The fp64 formulation against the stored fp64 run: 1e-9 relative plus the stored
copy's quantisation (an fp16 distance to the fp32 run: 2^-10 of the tensor's largest distance per element).
"""
import ctypes

import numpy as np
import pytest
import torch

import tgn_inputs as TI
import tgn_train_inputs as TT
import tgn_train_ref as TR
from tests.test_graphmixer_oracle import ATOL, RTOL

DTYPES = {"32": torch.float32, "64": torch.float64}
_runs = {}


def run(case, tag):
    """The formulation's four steps on the golden slices, computed once per (case, precision)."""
    if (case, tag) not in _runs:
        m = TT.build_model(case)
        ref = TR.RefTGN(m.state_dict(), TT.heads(case), DTYPES[tag])
        _runs[case, tag] = (ref, TR.train_steps(ref, TT.step_batches()), TT.shapes_of(m))
    return _runs[case, tag]


@pytest.mark.parametrize("tag", ["32", "64"])
@pytest.mark.parametrize("case", list(TT.CASES))
def test_formulation_matches_reference_steps(case, tag):
    g = TT.golden()
    _, outs, shapes = run(case, tag)
    for k, (loss, pos, neg, grads) in enumerate(outs):
        ref_loss, ref_logits, names, ref_grads, ref_norms = TT.stored(g, case, k, tag, shapes)
        _, _, _, g32, n32 = TT.stored(g, case, k, "32", shapes)
        _, _, _, g64, n64 = TT.stored(g, case, k, "64", shapes)
        got = torch.cat([pos, neg]).double().reshape(-1).numpy()
        if tag == "32":
            np.testing.assert_allclose(got, ref_logits, atol=ATOL, rtol=RTOL)
            np.testing.assert_allclose(float(loss), ref_loss, atol=ATOL, rtol=RTOL)
        else:
            np.testing.assert_allclose(got, ref_logits, atol=1e-7, rtol=0)      # stored as fp32
            np.testing.assert_allclose(float(loss), ref_loss, atol=1e-12, rtol=0)
        # exactly the tensors the reference's step fills: step 0 has no pending message, so the message MLP and
        # the GRU cell get no gradient there; a third attention layer never does
        have = {n for n, v in grads.items() if v is not None and n in shapes}
        assert have == set(names), (k, have ^ set(names))
        assert len(names) == (28 if k == 0 else 36)
        for n, ref in ref_grads.items():
            err, nref = float(torch.linalg.norm(grads[n].double() - ref)), float(torch.linalg.norm(ref))
            env = g32[n] - g64[n]
            if tag == "32":
                bound = max(1e-5 * nref, 3 * float(torch.linalg.norm(env)))
            else:
                bound = 1e-9 * nref + 2.0 ** -10 * float(env.abs().max()) * np.sqrt(ref.numel())
            assert err <= bound, (case, tag, k, n, err, bound, nref)
        for n, ref in ref_norms.items():
            got_n = float(torch.linalg.norm(grads[n].double()))
            bound = max(1e-5 * ref, 3 * abs(n32[n] - n64[n])) if tag == "32" else 1e-9 * ref
            assert abs(got_n - ref) <= bound, (case, tag, k, n, got_n, ref)


@pytest.mark.parametrize("case", list(TT.CASES))
def test_formulation_reaches_the_reference_state(case):
    """After the four steps: last_update, the nodes with a pending message and their timestamps equal the
    reference's; the memory, the last raw messages, the frozen model's logits of the whole batch on that state and
    the logits of the stateful eval() pass are the reference's within ATOL / RTOL."""
    g = TT.golden()
    ref, _, _ = run(case, "32")
    pre = f"{case}_end_"
    assert np.array_equal(ref.last_update.numpy(), g[pre + "last_update"])
    nodes = torch.nonzero(ref.msg_flag).reshape(-1)
    assert np.array_equal(nodes.numpy(), g[pre + "msg_nodes"])
    assert np.array_equal(ref.msg_ts[nodes].numpy(), g[pre + "msg_ts"])
    rows = torch.from_numpy(g[pre + "mem_rows"])
    assert np.array_equal(torch.nonzero(ref.memory.abs().sum(1)).reshape(-1).numpy(), rows.numpy())
    np.testing.assert_allclose(ref.memory[rows].numpy(), g[pre + "mem32"], atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(ref.msg_raw[nodes].numpy(), g[pre + "msg_raw32"], atol=ATOL, rtol=RTOL)
    pos, neg = ref.frozen(TT.full_batch())
    np.testing.assert_allclose(torch.cat([pos, neg]).numpy(), g[pre + "frozen32"], atol=ATOL, rtol=RTOL)
    # the reference's own fp32 error on this state (what the GPU bounds are taken from) is tiny
    assert float(g[pre + "mem_env"]) < 1e-5 and float(g[pre + "msg_raw_env"]) < 1e-5
    ev = TR.RefTGN(TT.build_model(case).state_dict(), TT.heads(case), torch.float32)
    with torch.no_grad():
        for k, batch in enumerate(TT.step_batches()):
            pos, neg = ev.step(batch)
            np.testing.assert_allclose(pos.numpy(), g[f"{case}_eval_s{k}_pos"], atol=ATOL, rtol=RTOL)
            np.testing.assert_allclose(neg.numpy(), g[f"{case}_eval_s{k}_neg"], atol=ATOL, rtol=RTOL)


def test_golden_slices_hold_the_hard_cases():
    """In-batch duplicate endpoints (steps 0-2), nodes that are both a source and a destination (step 0), and, from
    step 1 on, roots (2 / 2 / 10) and neighbours (11 / 23 / 32) with messages pending from the steps before."""
    seen, facts = set(), []
    for b in TT.step_batches():
        src, dst = b[0].tolist(), b[1].tolist()
        roots = set(src + dst + b[2].astype(np.int64).tolist())
        ngh = set(np.concatenate([sg[0][h].reshape(-1) for sg in b[5:8] for h in (0, 1)]).astype(np.int64).tolist())
        facts.append((len(src + dst) - len(set(src + dst)), len(set(src) & set(dst)), len(roots & seen),
                      len((ngh - {0}) & seen)))
        seen |= set(src + dst)
    assert facts == [(4, 2, 0, 0), (1, 0, 2, 11), (1, 0, 2, 23), (0, 0, 10, 32)]


def test_keep_masks_layout():
    """All-ones masks with scale 1 are the no-dropout step; zeroing the bytes of one (row, head) pair of layer 1 on
    the src side moves the logits of that event alone; a zeroed fc mask of layer 0 leaves that layer's fc without a
    gradient and layer 1's with one."""
    case = "small8"
    m = TT.build_model(case)
    sd, H, batch = m.state_dict(), TT.heads(case), TT.step_batches()[0]
    B, N, dq = TT.STEP_B, TI.N_DEG, 2 * m.n_node_features
    R1 = 3 * B
    shapes = [(R1 * N * H * N,), (R1 * H * N,), (R1 * N, dq), (R1, dq)]
    assert [tuple(s) for s in m.keep_mask_shapes(R1, N)] == shapes
    ones = [torch.ones(s, dtype=torch.uint8) for s in shapes]

    def logits(keep):
        ref = TR.RefTGN(sd, H)
        out = TR.train_steps(ref, [batch], None if keep is None else [keep], 1.0)[0]
        return torch.cat([out[1], out[2]]).reshape(-1), out[3]
    l0, _ = logits(None)
    l1, _ = logits(ones)
    assert torch.equal(l0, l1)
    k = [x.clone() for x in ones]
    row, head = 5, 1
    k[1].view(R1, H, N)[row, head] = 0
    l2, _ = logits(k)
    moved = (l2 - l0).abs() > 0
    assert moved[row] and moved[B + row] and int(moved.sum()) == 2      # src row 5 feeds its pos and its neg logit
    k = [x.clone() for x in ones]
    k[2][:] = 0
    _, grads = logits(k)
    pre = "embedding_module.attention_models."
    assert float(grads[pre + "0.multi_head_target.fc.weight"].abs().max()) == 0.0
    assert float(grads[pre + "1.multi_head_target.fc.weight"].abs().max()) > 0.0


def test_closed_form_backward_equals_autograd():
    """The fp64 closed form the kernel tests hold the training pair to (tgn_train_ref.attn_closed_form) against
    autograd through the forward formula: queries, explanation weights, the time parameters, the dense neighbour
    rows and the rows of a gathered table."""
    for case in (TT.KERNEL_CASES[1], TT.KERNEL_CASES[4]):
        x = TT.kernel_inputs(case, seed=11)
        ref = TR.attn_closed_form(x, x.keep, x.scale)
        Rr, N, H = x.R, x.N, x.H
        if x.dense:
            leaf = x.node.double().requires_grad_(True)
            node = leaf
        else:
            leaf = x.tab.double().requires_grad_(True)
            node = leaf[x.node_idx.long()]
        qf = x.qf.double().requires_grad_(True)
        tw, tb = x.tw.double().requires_grad_(True), x.tb.double().requires_grad_(True)
        ew = (torch.ones(Rr, N, dtype=torch.float64) if x.ew is None else x.ew.double()).requires_grad_(True)
        u = TR.time_arg(x.dt, x.tw, x.tb)                         # the rounded argument; its slope is the exact one's
        arg = x.dt.double().unsqueeze(-1) * tw + tb
        tf = torch.cos(u + (arg - arg.detach()))
        key = torch.cat([node, x.edge.double(), tf], dim=-1)
        m = TR.pair_rows(Rr, H, x.seg)
        s = torch.einsum("rhc,rjc->rhj", qf, key) / x.T
        p = torch.softmax(s.masked_fill(x.mask[m] == 0, -1e10), dim=-1)
        z = torch.einsum("rhj,rjc->rhc", p * ew[m] * (x.keep.view(Rr, H, N).double() * x.scale), key)
        (z * x.gz.double()).sum().backward()
        d_ew = torch.zeros(Rr, N, dtype=torch.float64).index_put_((m.reshape(-1),), ref.d_ew.reshape(Rr * H, N),
                                                                  accumulate=True)
        checks = [("z", ref.z, z.detach()), ("d_qf", ref.d_qf, qf.grad), ("d_ew", d_ew, ew.grad),
                  ("d_w", ref.d_time[0], tw.grad), ("d_b", ref.d_time[1], tb.grad),
                  ("d_node" if x.dense else "d_tab", ref.d_node if x.dense else ref.d_tab, leaf.grad)]
        for name, got, want in checks:
            scale = max(1.0, float(want.abs().max()))
            assert float((got - want).abs().max()) <= 1e-11 * scale, (case, name)
        assert bool((ref.mag_time >= ref.d_time.abs() * (1 - 1e-12)).all())
        # the per-(slot, head) scalars give every slot's key gradient: dk_j = sum_h a gz_h + b qf_h
        dk = torch.einsum("rjh,rhc->rjc", ref.a, x.gz.double()) + torch.einsum("rjh,rhc->rjc", ref.b, x.qf.double())
        assert float((dk[..., :x.dims[0]] - ref.d_node).abs().max()) <= 1e-12


def test_library_exports_the_training_pair():
    from tempme_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tm_tgn_attn_train_fwd", "tm_tgn_attn_train_bwd", "tm_tgn_attn_train_workspace_bytes",
                 "tm_tgn_attn_train_dtab", "tm_tgn_rows_reduce"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    wb = lib.tm_tgn_attn_train_workspace_bytes
    wb.restype = ctypes.c_int64
    wb.argtypes = [ctypes.c_int64, ctypes.c_int32]
    # one [2][d_time] partial per workgroup of four rows, at most 1024 workgroups however many rows
    assert wb(15, 8) == 4 * 4 * 2 * 8
    assert wb(4096, 172) == 1024 * 2 * 172 * 4
    assert 0 < wb(3 * 512 * 20, 172) <= 1024 * 2 * 172 * 4
    assert wb(0, 172) == 0 and wb(-1, 172) == -1


def test_model_and_memory_interface():
    from tempme_amd.tgn import TGN, Memory
    for name in ("train_on_hip", "draw_keep_masks", "keep_mask_shapes", "messages_to_dict", "messages_from_dict",
                 "pending_messages"):
        assert callable(getattr(TGN, name, None)), name
    for name in ("set_memory", "backup_memory", "restore_memory", "detach_memory"):
        assert callable(getattr(Memory, name, None)), name
    m = TT.build_model("small8", dropout=0.1)
    assert m.forbidden_memory_update is False
    assert m.train_on_hip() is m and m._train_on_hip is True
    assert m.train_on_hip(False)._train_on_hip is False
    # the state_dict keeps the reference's keys (tgn_uslegis.npz lists them): a reference checkpoint loads strictly
    g = TI.golden()
    ref_keys = {k[len("synth_sd_"):] for k in g.files if k.startswith("synth_sd_")}
    assert set(TI.build_model("synth").state_dict()) == ref_keys
    assert set(m.state_dict()) == ref_keys


def test_memory_backup_restore_detach():
    m = TT.build_model("small8")
    mem = m.memory
    mem.set_memory([2, 5], torch.ones(2, m.memory_dimension))
    mem.messages[3] = [(torch.arange(4.0).requires_grad_(True) * 2, torch.tensor(7.0))]
    b = mem.backup_memory()
    mem.set_memory([2], torch.zeros(1, m.memory_dimension))
    mem.last_update.data[4] = 9.0
    mem.clear_messages([3])
    mem.restore_memory(b)
    assert float(mem.memory[2].sum()) == m.memory_dimension and float(mem.last_update[4]) == 0.0
    assert len(mem.messages[3]) == 1 and float(mem.messages[3][0][1]) == 7.0
    assert mem.messages[3][0][0] is not b[2][3][0][0], "restore clones"
    assert mem.messages[3][0][0].requires_grad is False or mem.messages[3][0][0].grad_fn is not None
    mem.detach_memory()
    assert mem.messages[3][0][0].grad_fn is None and not mem.messages[3][0][0].requires_grad


def test_unsupported_options_are_named():
    """The stateful path restates learn_base.py's configuration; anything else raises and names the option (before
    any device work, so this runs without one)."""
    from tempme_amd.tgn import TGN
    nf, ef = TT.case_feats("small8")
    b = TT.step_batches()[0]
    for kw, name in ((dict(aggregator_type="mean"), "aggregator_type"),
                     (dict(memory_update_at_start=False), "memory_update_at_start"),
                     (dict(message_function="identity"), "message_function"),
                     (dict(memory_updater_type="rnn"), "memory_updater_type"),
                     (dict(use_source_embedding_in_message=False), "use_source_embedding_in_message"),
                     (dict(use_destination_embedding_in_message=False), "use_destination_embedding_in_message")):
        m = TGN(nf, ef, n_neighbors=TI.N_DEG, device=torch.device("cpu"), n_layers=2, **kw)
        with pytest.raises(NotImplementedError, match=name):
            m.contrast(*b)
        with pytest.raises(NotImplementedError, match=name):
            m.get_node_emb(*b)
    m = TGN(nf, ef, n_neighbors=TI.N_DEG, device=torch.device("cpu"), n_layers=2, aggregator_type="mean")
    m.memory.messages[1] = [(torch.zeros(m._raw_dim()), torch.tensor(1.0))] * 2
    with pytest.raises(NotImplementedError, match="mean"):
        m.messages_from_dict(torch.device("cpu"))


def test_learn_base_switch():
    from tempme_amd import learn_base
    for extra in ([], ["--n_layer", "3"], ["--n_layer", "1"]):
        with pytest.raises(NotImplementedError) as e:
            learn_base.main(["--base_type", "tgn", "-d", "uslegis_sampled"] + extra)
        msg = str(e.value)
        assert "tgn" in msg and "GraphMixer" in msg and "--n_layer 2" in msg and "2-hop" in msg
    # --n_layer 2 gets past the switch: the next thing it wants is the data set
    with pytest.raises(FileNotFoundError):
        learn_base.main(["--base_type", "tgn", "--n_layer", "2", "-d", "uslegis_sampled", "--data_dir",
                         "no_such_directory"])
    assert "tgn" in learn_base.__doc__ and "backup_memory" in learn_base.__doc__
