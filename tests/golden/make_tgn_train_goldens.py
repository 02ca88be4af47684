"""Generate tests/golden/tgn_train.npz by running the REFERENCE base TGN's stateful training steps on the CPU.

    python tests/golden/make_tgn_train_goldens.py <path to a checkout of dharunm236/TempME>

Run where the reference is available; the tests only read the committed .npz.  Nothing of the reference is
stored but what its programs compute: losses, logits, gradients, gradient norms, memory state and parameter names.

Inputs are the golden batch of tests/tgn_inputs.py (32 test events of uslegis_sampled at N = 20) run as 4
consecutive steps of 8 events: the slices hold in-batch duplicate endpoints, step 0 has nodes that are both a source
and a destination, and from step 1 on roots and neighbours have messages pending from the steps before.  Per case:
  * ``torch.manual_seed(seed); TGN(nf, ef, 20, n_layers=3, n_heads=H, dropout=0.0)`` in ``.train()`` mode with the
    reference's default ``forbidden_memory_update=False``; ``time_encoder.w.bias`` set to the committed perturbation
    of tgn_uslegis.npz cut to the time dimension;
  * per step ``zero_grad``, ``contrast`` (learn_base.py:227-232), the loss of learn_base.py:233-235, ``backward``,
    NO optimizer step (the weights stay fixed, so the steps are comparable), ``memory.detach_memory()``;
  * by the fp32 model (``..._32``) and by the same model cast to fp64 (``..._64``, stored as fp32 or as an fp16
    distance to the fp32 run: ``delta64`` times ``unit64``).  The fp64 model keeps ``last_update`` in fp32 (the
    reference writes fp32 timestamps into it) and gets one forward pre-hook on its time encoder that casts the
    (fp32-rounded) time offsets the reference builds to fp64: the same inputs, fp64 arithmetic.
Per step ``<case>_s<k>_``: loss, pos, neg, grad_names, and the gradients as one flat array in grad_names order
(small models: every gradient; full-size ``synth``: the 1-D gradients, and the matrices' Frobenius norms in
``norm32`` / ``norm64``, in grad_names order too); tests/tgn_train_inputs.py puts them back together.  After the last step ``<case>_end_``: the rows of ``memory`` that
are not zero, ``last_update``, the nodes with pending messages and their last raw message and timestamp (fp32 run;
of the fp64 run the largest distance to it, ``mem_env`` / ``msg_raw_env``), and the
``eval()`` / ``forbidden_memory_update=True`` logits of the whole 32-event batch on that state.
``<case>_eval_s<k>_pos / _neg``: a second run of the four slices in ``eval()`` under ``no_grad``, stateful, fp32.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tgn_inputs as TI  # noqa: E402

# case -> (d_node, d_edge (None = all columns of synth), heads, seed)
CASES = {"small8": (8, 4, 2, 41), "small10": (10, 5, 3, 42), "synth": (None, None, 2, 43)}
STEPS, STEP_B = 4, 8


def case_feats(case):
    dn, de, _, _ = CASES[case]
    nf, ef = TI.feats("synth")
    if dn is not None:
        nf, ef = np.ascontiguousarray(nf[:, :dn]), np.ascontiguousarray(ef[:, :de])
    return nf, ef


def case_bias(dim):
    return TI.golden()["synth_pert_time_bias"][:dim].copy()


def step_args(d, k):
    sl = slice(k * STEP_B, (k + 1) * STEP_B)
    sg = [tuple([x[sl] for x in part] for part in d["sg_" + s]) for s in TI.SIDES]
    return (d["src"][sl], d["dst"][sl], d["fake"][sl], d["ts_cut"][sl], d["e_idx"][sl], sg[0], sg[1], sg[2])


def build(TGN, case):
    nf, ef = case_feats(case)
    _, _, H, seed = CASES[case]
    torch.manual_seed(seed)
    m = TGN(nf, ef, n_neighbors=TI.N_DEG, device=torch.device("cpu"), n_layers=3, n_heads=H, dropout=0.0)
    with torch.no_grad():
        m.time_encoder.w.bias.data.copy_(torch.from_numpy(case_bias(m.n_node_features)))
    return m


def pending(m):
    nodes = sorted(int(k) for k, v in m.memory.messages.items() if len(v) > 0)
    raw = torch.stack([m.memory.messages[k][-1][0].detach() for k in nodes])
    ts = torch.stack([m.memory.messages[k][-1][1].detach().reshape(()) for k in nodes])
    return np.array(nodes, dtype=np.int64), raw, ts


def main(ref):
    sys.path.insert(0, ref)
    # stand-ins for modules the reference's TGN package imports and this run never calls (as make_goldens.py):
    # turtle (two unused names, TGN/tgn.py:2, embedding_module.py:1; it needs tkinter) and numba.jit (the sampler)
    if "turtle" not in sys.modules:
        stub = types.ModuleType("turtle")
        stub.pos = stub.position = None
        sys.modules["turtle"] = stub
    try:
        import numba  # noqa: F401
    except ImportError:
        stub = types.ModuleType("numba")
        stub.jit = lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f))
        sys.modules["numba"] = stub
    from TGN.tgn import TGN
    d = TI.load_batch()
    full = (d["src"], d["dst"], d["fake"], d["ts_cut"], d["e_idx"], d["sg_src"], d["sg_tgt"], d["sg_bgd"])
    crit = torch.nn.BCEWithLogitsLoss()
    res = {}
    for case, (dn, _, _, _) in CASES.items():
        small = dn is not None
        base = build(TGN, case).train()
        m64 = copy.deepcopy(base).double()
        # timestamps stay fp32 in both runs (the reference stores them as fp32 tensors and index_puts them)
        m64.memory.last_update.data = m64.memory.last_update.data.float()
        m64.time_encoder.register_forward_pre_hook(lambda mod, a: (a[0].to(mod.w.weight.dtype),))
        for tag, m in (("32", base), ("64", m64)):
            for k in range(STEPS):
                pre = f"{case}_s{k}_"
                m.zero_grad()
                pos, neg = m.contrast(*step_args(d, k))
                loss = crit(pos, torch.ones_like(pos)) + crit(neg, torch.zeros_like(neg))
                loss.backward()
                m.memory.detach_memory()
                res[f"{pre}loss{tag}"] = np.array(loss.item(), dtype=np.float64)
                res[f"{pre}pos{tag}"] = pos.detach().to(torch.float32).numpy()
                res[f"{pre}neg{tag}"] = neg.detach().to(torch.float32).numpy()
                # one flat array per step: the gradients stored in full, in grad_names order (a zip entry per
                # tensor would cost more than the numbers); matrices of the full-size model go as Frobenius norms
                names, flat, norms = [], [], []
                for name, v in m.named_parameters():
                    if v.grad is None:
                        continue
                    names.append(name)
                    g = v.grad.detach()
                    if small or g.dim() == 1:
                        flat.append(g.double().reshape(-1).numpy())
                    else:
                        norms.append(torch.linalg.norm(g.double()).item())
                if tag == "32":
                    res[f"{pre}grad_names"] = np.array(names)
                    res[f"{pre}grad32"] = np.concatenate(flat).astype(np.float32)
                else:
                    assert list(res[f"{pre}grad_names"]) == names
                    # fp64 gradients as their fp16 distance to the fp32 ones, per tensor in units of its largest
                    # distance (5e-4 of a distance that is itself ~1e-6 of the gradient: finer than an fp32 copy)
                    g32, off, deltas, units = res[f"{pre}grad32"].astype(np.float64), 0, [], []
                    for v in flat:
                        delta = v - g32[off:off + len(v)]
                        off += len(v)
                        units.append(float(np.abs(delta).max()) or 1.0)
                        deltas.append((delta / units[-1]).astype(np.float16))
                    res[f"{pre}grad_delta64"] = np.concatenate(deltas)
                    res[f"{pre}grad_unit64"] = np.array(units)
                res[f"{pre}norm{tag}"] = np.array(norms, dtype=np.float64)
                print(case, tag, "step", k, "loss", loss.item(), "params with grad", len(names))
            # the state after the last step
            pre = f"{case}_end_"
            mem = m.memory.memory.detach().numpy()
            nodes, raw, ts = pending(m)
            if tag == "32":
                rows = np.nonzero(np.abs(mem).sum(1))[0].astype(np.int64)
                res[pre + "mem_rows"], res[pre + "mem32"] = rows, mem[rows].copy()
                res[pre + "last_update"] = m.memory.last_update.detach().numpy().copy()
                res[pre + "msg_nodes"], res[pre + "msg_raw32"], res[pre + "msg_ts"] = nodes, raw.numpy().copy(), ts.numpy().copy()
            else:
                rows = res[pre + "mem_rows"]
                assert np.array_equal(np.nonzero(np.abs(mem).sum(1))[0], rows) and np.array_equal(nodes, res[pre + "msg_nodes"])
                assert np.array_equal(m.memory.last_update.detach().numpy().astype(np.float32), res[pre + "last_update"])
                assert np.array_equal(ts.numpy().astype(np.float32), res[pre + "msg_ts"])
                # the reference's own fp32 error on the state: the largest distance between its two runs
                res[pre + "mem_env"] = np.array(np.abs(mem[rows] - res[pre + "mem32"]).max())
                res[pre + "msg_raw_env"] = np.array(np.abs(raw.numpy() - res[pre + "msg_raw32"]).max())
            m.forbidden_memory_update = True
            m.eval()
            with torch.no_grad():
                pos, neg = m.contrast(*full)
            res[f"{pre}frozen{tag}"] = torch.cat([pos, neg]).to(torch.float32).numpy()
        # the stateful evaluation pass (learn_base.py:43-73): eval(), no_grad, the memory moving on batch by batch
        ev = build(TGN, case).eval()
        with torch.no_grad():
            for k in range(STEPS):
                pos, neg = ev.contrast(*step_args(d, k))
                res[f"{case}_eval_s{k}_pos"], res[f"{case}_eval_s{k}_neg"] = pos.numpy().copy(), neg.numpy().copy()
    out = os.path.join(HERE, "tgn_train.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
