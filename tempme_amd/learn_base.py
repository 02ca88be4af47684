"""Stage one of the reference's workflow, ``learn_base.py``, for its three base models:
train the base model that ``temp_exp_main.py`` explains and ``enhance_main.py`` enhances.

    python -m tempme_amd.learn_base -d uslegis_sampled --data_dir processed --base_type graphmixer
    python -m tempme_amd.learn_base -d uslegis_sampled --data_dir processed --base_type tgat --n_layer 2
    python -m tempme_amd.learn_base -d uslegis_sampled --data_dir processed --base_type tgn --n_layer 2

restates learn_base.py: the chronological 0.70 / 0.85 split with 10 % of the later nodes masked out of training
(:90-152), the training loop (:201-253), the evaluation (:43-73), early stopping on the test AP and the saved
best model.  The training step runs on the HIP path of ``GraphMixer.train_on_hip()`` (tm_gm_train_fwd /
tm_gm_train_bwd, csrc/graphmixer_train.hip); subgraphs come from the device ``NeighborFinder.find_k_hop`` and
negatives from the device ``RandEdgeSampler`` (keyed draws: a seed reproduces an epoch exactly).  With
``--base_type tgat`` the step runs on ``TGAT.train_on_hip()`` (tm_tgat_attn_train_fwd / tm_tgat_attn_train_bwd,
csrc/tgat_train.hip) over 2-hop subgraphs; TGAT is built for ``--n_layer 2`` only.

With ``--base_type tgn`` the step runs on ``TGN.train_on_hip()`` (tm_tgn_attn_train_fwd / tm_tgn_attn_train_bwd /
tm_tgn_attn_train_dtab, csrc/tgn_train.hip) with the stateful memory on the device: every step applies the pending
messages, persists the positives' memory and stores the batch's raw messages (TGN/tgn.py:123-196), and
``memory.detach_memory()`` follows ``optimizer.step()``.  As in the reference the memory is never re-initialised
between epochs, and each epoch's evaluation (which moves the memory on, batch by batch) runs between
``backup_memory()`` and ``restore_memory()``.  TGN reads 2-hop subgraphs, so ``--n_layer 2`` is required.  Next to
the best model's ``state_dict`` (``<prefix>tgn_<data>.pt``) the pending messages of the training memory are saved
as ``<prefix>tgn_<data>_messages.pt`` ({"nodes", "raw", "ts"} tensors; ``TGN.load_pending_messages`` reads them).
"""
import argparse
import math
import os
import random
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L
from .tgat import TGAT
from .tgn import TGN

degree_dict = {"wikipedia": 20, "reddit": 20, "uci": 30, "mooc": 60, "enron": 30, "enron_sampled": 30, "canparl": 30,
               "uslegis": 30, "uslegis_sampled": 30}


class EarlyStopMonitor:
    """utils/batch_loader.py:4-29."""

    def __init__(self, max_round=3, higher_better=True, tolerance=1e-3):
        self.max_round = max_round
        self.num_round = 0
        self.epoch_count = 0
        self.best_epoch = 0
        self.last_best = None
        self.higher_better = higher_better
        self.tolerance = tolerance

    def early_stop_check(self, curr_val):
        self.epoch_count += 1
        if not self.higher_better:
            curr_val *= -1
        if self.last_best is None:
            self.last_best = curr_val
        elif (curr_val - self.last_best) / np.abs(self.last_best) > self.tolerance:
            self.last_best = curr_val
            self.num_round = 0
            self.best_epoch = self.epoch_count
        else:
            self.num_round += 1
        return self.num_round >= self.max_round


def split_data(g_df, seed=2023, device=None, finders=True, sampler_seed=0):
    """learn_base.py:90-152.  g_df: the ``ml_<data>.csv`` table (a DataFrame, or any mapping with the columns u, i,
    ts, label, idx).  Returns a namespace with val_time / test_time (the 0.70 / 0.85 time quantiles),
    mask_node_set (10 % of all nodes, drawn from those seen after val_time with ``random.seed(seed)``), the
    train / val / test columns (``train_src_l`` ...), and -- with finders=True, which needs the HIP device --
    train_ngh_finder / full_ngh_finder and train_rand_sampler / test_rand_sampler."""
    src_l, dst_l = np.asarray(g_df["u"]), np.asarray(g_df["i"])
    e_idx_l, label_l, ts_l = np.asarray(g_df["idx"]), np.asarray(g_df["label"]), np.asarray(g_df["ts"])
    val_time, test_time = list(np.quantile(ts_l, [0.70, 0.85]))
    max_idx = int(max(src_l.max(), dst_l.max()))
    random.seed(seed)
    total_node_set = set(np.unique(np.hstack([src_l, dst_l])))
    num_total_unique_nodes = len(total_node_set)
    later = list(set(src_l[ts_l > val_time]).union(set(dst_l[ts_l > val_time])))
    mask_node_set = set(random.sample(later, int(0.1 * num_total_unique_nodes)))
    masked = np.fromiter(mask_node_set, dtype=src_l.dtype, count=len(mask_node_set))
    none_node_flag = ~np.isin(src_l, masked) & ~np.isin(dst_l, masked)
    flags = {"train": (ts_l <= val_time) & none_node_flag, "val": (ts_l <= test_time) & (ts_l > val_time),
             "test": ts_l > test_time}
    s = SimpleNamespace(val_time=val_time, test_time=test_time, mask_node_set=mask_node_set, max_idx=max_idx,
                        src_l=src_l, dst_l=dst_l, ts_l=ts_l, e_idx_l=e_idx_l, label_l=label_l)
    for name, f in flags.items():
        for col, arr in (("src", src_l), ("dst", dst_l), ("ts", ts_l), ("e_idx", e_idx_l), ("label", label_l)):
            setattr(s, f"{name}_{col}_l", arr[f])
    if finders:
        from .batch_loader import RandEdgeSampler
        from .graph import NeighborFinder
        dev = L.require_device(device)
        s.train_ngh_finder = NeighborFinder.from_edges(s.train_src_l, s.train_dst_l, s.train_e_idx_l, s.train_ts_l,
                                                       max_idx + 1, device=dev, seed=sampler_seed,
                                                       split=L.SPLIT_TRAIN)
        s.full_ngh_finder = NeighborFinder.from_edges(src_l, dst_l, e_idx_l, ts_l, max_idx + 1, device=dev,
                                                      seed=sampler_seed, split=L.SPLIT_TEST)
        s.train_rand_sampler = RandEdgeSampler((s.train_src_l,), (s.train_dst_l,), seed=sampler_seed,
                                               split=L.SPLIT_TRAIN, device=dev)
        s.test_rand_sampler = RandEdgeSampler((s.train_src_l, s.val_src_l, s.test_src_l),
                                              (s.train_dst_l, s.val_dst_l, s.test_dst_l), seed=sampler_seed,
                                              split=L.SPLIT_TEST, device=dev)
    return s


def _is_tgat(base_model):
    return isinstance(base_model, TGAT)


def _is_tgn(base_model):
    return isinstance(base_model, TGN)


def _contrast(base_model, batch):
    """learn_base.py:227-232: TGAT takes if_explain, GraphMixer and TGN explain_weights / edge_attr."""
    a = (batch.src, batch.dst, batch.fake, batch.ts, batch.e_idx, batch.sg_src, batch.sg_tgt, batch.sg_bgd)
    if _is_tgat(base_model):
        return base_model.contrast(*a, if_explain=False)
    return base_model.contrast(*a, explain_weights=None, edge_attr=None)


def make_batch(base_model, sampler, src, dst, ts, e_idx=None, event_ids=None):
    """One batch as learn_base.py:215-226 assembles it: the negative destinations and the three sides'
    subgraphs (device tensors; GraphMixer reads hop 1 only, TGAT samples its num_layers hops, TGN 2 hops)."""
    size = len(src)
    ev = None if event_ids is None else np.asarray(event_ids, dtype=np.int64)
    _, fake = sampler.sample(size, event_ids=ev, as_tensor=True)
    fake_np = fake.cpu().numpy()
    tgat, tgn = _is_tgat(base_model), _is_tgn(base_model)
    if tgn:
        finder = base_model.embedding_module.neighbor_sampler
    else:
        finder = base_model.ngh_finder if tgat else base_model.neighbor_sampler
    N = base_model.num_neighbors
    sgs = [finder.find_k_hop(2 if tgn else base_model.num_layers if tgat else 1, roots, ts, N, e_idx_l=None, event_ids=ev, side=side, as_tensor=True)
           for roots, side in ((src, L.SIDE_SRC), (dst, L.SIDE_TGT), (fake_np, L.SIDE_BGD))]
    # everything the step reads is on the device already: train_step then copies nothing from the host and waits for nothing
    dev = finder.device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    return SimpleNamespace(src=t(src, torch.long), dst=t(dst, torch.long), fake=fake.long(), ts=t(ts, torch.float64),
                           e_idx=e_idx, sg_src=sgs[0], sg_tgt=sgs[1], sg_bgd=sgs[2], size=size)


def train_step(base_model, optimizer, batch):
    """learn_base.py:223-237 on a prepared batch: zero_grad, contrast, BCEWithLogits(pos, 1) +
    BCEWithLogits(neg, 0), backward, step.  Returns (loss, pos, neg) as device tensors; nothing here waits for
    the device."""
    optimizer.zero_grad()
    pos, neg = _contrast(base_model, batch)
    crit = torch.nn.functional.binary_cross_entropy_with_logits
    loss = crit(pos, torch.ones_like(pos)) + crit(neg, torch.zeros_like(neg))
    loss.backward()
    optimizer.step()
    if _is_tgn(base_model):
        base_model.memory.detach_memory()       # learn_base.py:238-239
    return loss.detach(), pos.detach(), neg.detach()


def _metrics(pos, neg):
    from sklearn.metrics import average_precision_score, roc_auc_score
    score = np.concatenate([pos.sigmoid().reshape(-1).cpu().numpy(), neg.sigmoid().reshape(-1).cpu().numpy()])
    size = len(score) // 2
    true = np.concatenate([np.ones(size), np.zeros(size)])
    return ((score > 0.5) == true).mean(), average_precision_score(true, score), roc_auc_score(true, score)


def _metrics_device(outs):
    """``_metrics`` of every (pos, neg) pair as one float64 [steps, 3] array (acc, ap, auc), computed on the
    device: the pairs of one batch size are stacked into [steps, 2B] scores against the labels [1...1, 0...0]
    and go through one ``metrics.rank_metrics`` launch (a shorter last batch gets its own); one copy to the host
    at the end."""
    from .metrics import rank_metrics
    if not outs:
        return np.zeros((0, 3))
    groups = {}
    for k, (pos, neg) in enumerate(outs):
        score = torch.cat([pos.detach().sigmoid().reshape(-1), neg.detach().sigmoid().reshape(-1)])
        groups.setdefault(int(score.numel()), []).append((k, score))
    res = torch.empty((len(outs), 3), dtype=torch.float64, device=outs[0][0].device)
    for n2, members in groups.items():
        score = torch.stack([s for _, s in members])
        true = torch.cat([torch.ones(n2 // 2, device=score.device), torch.zeros(n2 - n2 // 2, device=score.device)])
        acc = ((score > 0.5) == (true > 0.5)).sum(1, dtype=torch.float64) / n2
        rows = torch.tensor([k for k, _ in members], dtype=torch.int64).to(score.device, non_blocking=True)
        res[rows] = torch.cat([acc.reshape(-1, 1), rank_metrics(true, score)], dim=1)
    return res.cpu().numpy()


def train_epoch(base_model, optimizer, finder, sampler, src, dst, ts, e_idx, bs, *, idx_list=None, max_steps=None,
                event_base=0, metrics=True, device_metrics=False):
    """learn_base.py:201-253: one pass over the training edges in the order of idx_list (default: a fresh
    np.random shuffle, as the reference).  Returns {"loss": [...], "acc", "ap", "auc"}; the per-step losses
    are read back once, at the end of the epoch.  ``device_metrics``: acc / ap / auc of every step from the
    device (``_metrics_device``) instead of scikit-learn on the host."""
    base_model.train()
    base_model.set_neighbor_sampler(finder)
    num_instance = len(src)
    num_batch = math.ceil(num_instance / bs)
    if idx_list is None:
        idx_list = np.arange(num_instance)
        np.random.shuffle(idx_list)
    losses, outs = [], []
    for k in range(num_batch if max_steps is None else min(num_batch, max_steps)):
        s_idx = k * bs
        e = min(num_instance - 1, s_idx + bs)
        if s_idx >= e:
            continue
        rows = idx_list[s_idx:e]
        ev = event_base + s_idx + np.arange(len(rows))
        batch = make_batch(base_model, sampler, src[rows], dst[rows], ts[rows], e_idx[rows], event_ids=ev)
        loss, pos, neg = train_step(base_model, optimizer, batch)
        losses.append(loss)
        if metrics:
            outs.append((pos, neg))
    out = {"loss": [float(x) for x in torch.stack(losses).cpu()] if losses else []}
    if metrics and outs:
        m = _metrics_device(outs) if device_metrics else np.array([_metrics(p, n) for p, n in outs])
        out["acc"], out["ap"], out["auc"] = m.mean(axis=0)
    return out


def eval_one_epoch(args, base_model, sampler, src, dst, ts, label, val_e_idx_l=None):
    """learn_base.py:43-73 -> (acc, ap, None, auc), means over the batches (``args.device_metrics``: the
    batches' figures from ``_metrics_device`` at the end of the epoch)."""
    device_metrics = bool(getattr(args, "device_metrics", False))
    res = []
    with torch.no_grad():
        base_model = base_model.eval()
        num_test_instance = len(src)
        num_test_batch = math.ceil(num_test_instance / args.bs)
        for k in range(num_test_batch):
            s_idx = k * args.bs
            e_idx = min(num_test_instance - 1, s_idx + args.bs)
            if s_idx == e_idx:
                continue
            e_l_cut = val_e_idx_l[s_idx:e_idx] if (val_e_idx_l is not None) else None
            batch = make_batch(base_model, sampler, src[s_idx:e_idx], dst[s_idx:e_idx], ts[s_idx:e_idx], e_l_cut,
                               event_ids=s_idx + np.arange(e_idx - s_idx))
            pos, neg = _contrast(base_model, batch)
            res.append((pos, neg) if device_metrics else _metrics(pos, neg))
    acc, ap, auc = (_metrics_device(res) if device_metrics else np.array(res)).mean(axis=0)
    return acc, ap, None, auc


def parser():
    p = argparse.ArgumentParser("Interface for temporal GNN on future link prediction")
    p.add_argument("--base_type", type=str, default="graphmixer", help="tgn or graphmixer or tgat")
    p.add_argument("--gpu", type=int, default=0, help="idx for the gpu to use")
    p.add_argument("-d", "--data", type=str, help="data sources to use, try wikipedia or reddit", default="wikipedia")
    p.add_argument("--bs", type=int, default=512, help="batch_size")
    p.add_argument("--prefix", type=str, default="", help="prefix to name the checkpoints")
    p.add_argument("--n_degree", type=int, default=20, help="number of neighbors to sample")
    p.add_argument("--n_head", type=int, default=2, help="number of heads used in attention layer")
    p.add_argument("--n_epoch", type=int, default=100, help="number of epochs")
    p.add_argument("--n_layer", type=int, default=3, help="number of network layers")
    p.add_argument("--lr", type=float, default=0.01, help="learning rate")
    p.add_argument("--drop_out", type=float, default=0.5, help="dropout probability")
    p.add_argument("--node_dim", type=int, default=100, help="Dimentions of the node embedding")
    p.add_argument("--time_dim", type=int, default=100, help="Dimentions of the time embedding")
    # not in the reference: where ml_<data>.csv / .npy / _node.npy live and where the best model goes
    p.add_argument("--data_dir", type=str, default="processed")
    p.add_argument("--out_dir", type=str, default=os.path.join("params", "tgnn"))
    p.add_argument("--seed", type=int, default=0, help="seed of the keyed neighbour / negative draws")
    p.add_argument("--device_metrics", action="store_true",
                   help="acc / AP / AUC of every batch on the device (tm_rank_metrics) instead of scikit-learn")
    return p


def main(argv=None):
    import pandas as pd

    from .graphmixer import GraphMixer
    args = parser().parse_args(argv)
    if args.base_type == "tgn" and args.n_layer != 2:
        raise NotImplementedError(f"learn_base: --base_type tgn needs --n_layer 2 (got --n_layer {args.n_layer}): TGN "
                                  "reads 2-hop subgraphs and only two attention layers ever run, so a third would "
                                  "hold parameters the step never trains; only the GraphMixer base takes another "
                                  "depth")
    if args.base_type not in ("graphmixer", "tgat", "tgn"):
        raise ValueError(f"Wrong value for base_type {args.base_type}!")
    if args.base_type == "tgat" and args.n_layer != 2:
        # TGAT's own refusal (tgat.py), raised here before any file is read
        raise NotImplementedError(f"learn_base: --base_type tgat needs --n_layer 2 (got --n_layer {args.n_layer}): "
                                  f"num_layers {args.n_layer}: the explanation path samples 2-hop subgraphs, so only "
                                  "num_layers=2 is built; only the GraphMixer base takes another depth")
    args.n_degree = degree_dict.get(args.data, args.n_degree)
    g_df = pd.read_csv(os.path.join(args.data_dir, f"ml_{args.data}.csv"))
    e_feat = np.load(os.path.join(args.data_dir, f"ml_{args.data}.npy"))
    n_feat = np.load(os.path.join(args.data_dir, f"ml_{args.data}_node.npy"))
    args.device = L.require_device(torch.device("cuda", args.gpu))
    sp = split_data(g_df, device=args.device, sampler_seed=args.seed)
    if args.base_type == "tgat":
        base_model = TGAT(n_feat, e_feat, num_layers=args.n_layer, num_neighbors=args.n_degree, n_head=args.n_head,
                          drop_out=args.drop_out).to(args.device)
    elif args.base_type == "tgn":
        base_model = TGN(n_feat, e_feat, n_neighbors=args.n_degree, device=args.device, n_layers=args.n_layer,
                         n_heads=args.n_head, dropout=args.drop_out).to(args.device)
    else:
        base_model = GraphMixer(n_feat, e_feat, n_neighbors=args.n_degree, device=args.device,
                                num_tokens=args.n_degree, num_layers=args.n_layer, dropout=args.drop_out).to(args.device)
    base_model.train_on_hip()
    optimizer = torch.optim.Adam(base_model.parameters(), lr=args.lr)
    num_instance = len(sp.train_src_l)
    print(f"dataset:{args.data}, base_type model:{args.base_type}")
    print("num of training instances: {}".format(num_instance))
    print("num of batches per epoch: {}".format(math.ceil(num_instance / args.bs)))
    idx_list = np.arange(num_instance)
    best_aps = 0
    early_stopper = EarlyStopMonitor(max_round=5)
    for epoch in range(args.n_epoch):
        np.random.shuffle(idx_list)
        print("start {} epoch".format(epoch))
        tr = train_epoch(base_model, optimizer, sp.train_ngh_finder, sp.train_rand_sampler, sp.train_src_l,
                         sp.train_dst_l, sp.train_ts_l, sp.train_e_idx_l, args.bs, idx_list=idx_list,
                         event_base=epoch * num_instance, device_metrics=args.device_metrics)
        print("train acc: {}, train ap: {}, train auc:{}, loss: {}".format(tr.get("acc"), tr.get("ap"), tr.get("auc"),
                                                                          np.mean(tr["loss"])))
        base_model.set_neighbor_sampler(sp.full_ngh_finder)
        tgn = args.base_type == "tgn"
        if tgn:
            memory_backup = base_model.memory.backup_memory()      # the evaluation moves the memory on
        test_acc, test_ap, _, test_auc = eval_one_epoch(args, base_model, sp.test_rand_sampler, sp.test_src_l,
                                                        sp.test_dst_l, sp.test_ts_l, sp.test_label_l, sp.test_e_idx_l)
        if tgn:
            base_model.memory.restore_memory(memory_backup)        # never re-initialised: training goes on from here
        print("test acc: {}, test ap: {}, test auc: {}".format(test_acc, test_ap, test_auc))
        if test_ap > best_aps:
            os.makedirs(args.out_dir, exist_ok=True)
            path = os.path.join(args.out_dir, f"{args.prefix}{args.base_type}_{args.data}.pt")
            torch.save(base_model.state_dict(), path)
            if tgn:
                # the training memory is restored: its pending messages go next to the state_dict
                torch.save({k: v.cpu() for k, v in base_model.pending_messages().items()},
                           os.path.join(args.out_dir, f"{args.prefix}tgn_{args.data}_messages.pt"))
            print(f"save model to {path}")
            best_aps = test_ap
        if early_stopper.early_stop_check(test_ap):
            break
    return best_aps


if __name__ == "__main__":
    main()
