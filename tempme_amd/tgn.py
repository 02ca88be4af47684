"""Drop-in base ``TGN`` (TGN/tgn.py) for the consumer side of the explanation path.

TempME's training and evaluation loops hand the explanation to the frozen base model:
``base_model.contrast(src, dst, fake, ts, e_idx, sg_src, sg_tgt, sg_bgd, explain_weights=expl)``
(temp_exp_main.py:614-623, :306-321, threshold_test :153-272).  This module keeps the reference's
constructor, submodule names (a reference ``state_dict`` loads as is), construction order (so
``torch.manual_seed(s); TGN(...)`` draws the reference's initial weights) and the
``contrast`` / ``get_node_emb`` / ``grab_subgraph`` signatures.

``contrast`` runs on the HIP device:
  * per layer, the neighbour-facing part (key construction from the feature tables, scores for all
    heads, masked softmax, explanation weight, weighted key sum) is one launch of the attention forward
    (``attn_fwd_kernel`` / ``attn_fwd_split_kernel`` of csrc/attn_kernels.h, shared with TGAT, in their TGN
    instances; C ABI ``tm_tgn_attn_fwd``, autograd wrapper ``attn_op.AttnFn``);
  * the reference's per-neighbour projections fold into per-row ones: qf = (W_k^T W_q) query before
    the kernel and (fc W_v) z after it, two hipBLASLt GEMMs over source rows, followed by the
    residual LayerNorm and the merger MLP (torch ops on the device);
  * gradients with respect to the explanation weights (the explainer's training signal,
    temp_exp_main.py:624-631) come from ``attn_bwd_kernel`` (``tm_tgn_attn_bwd``) and torch
    autograd for the dense per-row algebra.  The base model is frozen: its parameters get no .grad.

Scope: the "graph_attention" embedding module, 2-hop subgraphs.  With ``forbidden_memory_update=True`` (the path
TempME uses, temp_exp_main.py:703-704) the model is frozen: memory messages stored on the model are applied through
get_updated_memory semantics (tgn.py:237-248) once per memory state.

With ``forbidden_memory_update=False`` (the constructor's default, as learn_base.py trains the base model) contrast
and get_node_emb are stateful as tgn.py:123-196: they embed over the updated memory, persist the positives' memory,
clear their messages and store the batch's raw messages.  The state lives on the device (``Memory.msg_raw`` /
``msg_ts`` / ``msg_flag``: under the ``last`` aggregator one raw message per node is all the reference reads) and
moves on without a loop over events and without a host synchronisation.  After ``train_on_hip()`` a ``train()``
step runs the training pair ``tm_tgn_attn_train_fwd`` / ``tm_tgn_attn_train_bwd`` (csrc/attn_train.h, entry
points in csrc/tgn_train.hip; ``attn_op.TrainAttnFn``) with the reference's two dropouts on the live parameters,
and ``loss.backward()`` fills ``.grad`` on every tensor the reference's step trains -- TimeEncode, the message MLP
and the GRU cell (through the updated memory rows the keys and queries gather: ``tm_tgn_attn_train_dtab`` /
``tm_tgn_rows_reduce``, no atomics), the two attention layers and ``affinity_score``.  ``messages_to_dict()`` /
``messages_from_dict()`` move the pending messages between the device store and ``memory.messages``, which the
frozen path reads (it calls the former itself when the store is newer).

The layer around the op is attn_layer.py's, shared with tgat.py (``fold``: this module multiplies by the ``.t()``
views of the row-major P, G; ``prep_inputs`` with ``sides=3`` and ``seg`` 0 for a single segment).  TGN's own: the
one-MergeLayer merger over [h | src], ``cos(time bias)`` as the query's time feature, ``keep_mask_shapes``, the
gathered node table with its gradient and the stateful memory.
"""
from collections import defaultdict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import attn_layer as AL
from .attn_layer import cat_rows as _cat_rows  # noqa: F401  (the name it had here: tests/test_tgn_cat_rows.py)
from .attn_op import AttnFn, TrainAttnFn, as_dev, attn_probs


# ------------------------------------------------------------------ modules (parameter layout)
class TimeEncode(nn.Module):
    """embedding_module.py:100-112: Linear(1, d) with frequencies 10^-linspace(0, 9, d), phase 0."""

    def __init__(self, dimension):
        super().__init__()
        self.dimension = dimension
        self.w = nn.Linear(1, dimension)
        freq = 1.0 / 10 ** np.linspace(0, 9, dimension)
        self.w.weight = nn.Parameter(torch.from_numpy(freq).float().reshape(dimension, -1))
        self.w.bias = nn.Parameter(torch.zeros(dimension).float())

    def forward(self, t):
        return torch.cos(self.w(t.unsqueeze(dim=2)))


class MergeLayer(nn.Module):
    """embedding_module.py:115-128: fc2(relu(fc1([x1 | x2])))."""

    def __init__(self, dim1, dim2, dim3, dim4):
        super().__init__()
        self.fc1 = nn.Linear(dim1 + dim2, dim3)
        self.fc2 = nn.Linear(dim3, dim4)
        self.act = nn.ReLU()
        nn.init.xavier_normal_(self.fc1.weight)
        nn.init.xavier_normal_(self.fc2.weight)

    def forward(self, x1, x2):
        return self.fc2(self.act(self.fc1(torch.cat([x1, x2], dim=1))))


class MultiHeadAttention(nn.Module):
    """Parameters of embedding_module.py:35-60 (d_k = d_v = key dim, no projection bias)."""

    def __init__(self, n_head, d_emb, d_k, d_v, dropout=0.1):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.w_qs = nn.Linear(d_emb, n_head * d_k, bias=False)
        self.w_ks = nn.Linear(d_k, n_head * d_k, bias=False)
        self.w_vs = nn.Linear(d_v, n_head * d_v, bias=False)
        nn.init.normal_(self.w_qs.weight, mean=0, std=np.sqrt(2.0 / (d_emb + d_k)))
        nn.init.normal_(self.w_ks.weight, mean=0, std=np.sqrt(2.0 / (d_emb + d_k)))
        nn.init.normal_(self.w_vs.weight, mean=0, std=np.sqrt(2.0 / (d_emb + d_v)))
        self.temperature = float(np.power(d_k, 0.5))
        self.fc = nn.Linear(n_head * d_v, d_emb)
        nn.init.xavier_normal_(self.fc.weight)
        self.layer_norm = nn.LayerNorm(d_emb)
        self.dropout = nn.Dropout(dropout)


class TemporalAttentionLayer(nn.Module):
    """embedding_module.py:130-166: query [node | time], key [node | edge | time]."""

    def __init__(self, n_node_features, n_neighbors_features, n_edge_features, time_dim, output_dimension,
                 n_head=2, dropout=0.1):
        super().__init__()
        self.n_head = n_head
        self.feat_dim = n_node_features
        self.time_dim = time_dim
        self.query_dim = n_node_features + time_dim
        self.key_dim = n_neighbors_features + time_dim + n_edge_features
        self.merger = MergeLayer(self.query_dim, n_node_features, n_node_features, output_dimension)
        self.multi_head_target = MultiHeadAttention(n_head=n_head, d_emb=self.query_dim, d_k=self.key_dim,
                                                    d_v=self.key_dim, dropout=dropout)


class Memory(nn.Module):
    """memory.py:8-75: per-node memory and last-update time (parameters, no grad) + raw messages."""

    def __init__(self, n_nodes, memory_dimension, input_dimension, message_dimension=None, device="cpu",
                 combination_method="sum"):
        super().__init__()
        self.n_nodes = n_nodes
        self.memory_dimension = memory_dimension
        self.input_dimension = input_dimension
        self.message_dimension = message_dimension
        self.device = device
        self.combination_method = combination_method
        self.__init_memory__()

    def __init_memory__(self):
        self.memory = nn.Parameter(torch.zeros((self.n_nodes, self.memory_dimension)), requires_grad=False)
        self.last_update = nn.Parameter(torch.zeros(self.n_nodes), requires_grad=False)
        self.messages = defaultdict(list)
        # the pending store of the stateful path (TGN.contrast with forbidden_memory_update=False): under the
        # ``last`` aggregator only a node's last raw message is ever read, so one row, its timestamp and a flag
        # per node hold what the reference's dict of lists holds.  ``store_is_newer``: the store has moved on
        # from ``messages`` (TGN.messages_to_dict() writes it back); else ``messages`` is what counts
        self.msg_raw = self.msg_ts = self.msg_flag = None
        self.store_is_newer = False
        self.store_any = False          # host-side: some node may have a pending message in the store

    def store_raw_messages(self, nodes, node_id_to_messages):
        for node in nodes:
            self.messages[node].extend(node_id_to_messages[node])

    def get_memory(self, node_idxs):
        return self.memory[node_idxs, :]

    def set_memory(self, node_idxs, values):
        """memory.py:42-43."""
        with torch.no_grad():
            self.memory[node_idxs, :] = values

    def get_last_update(self, node_idxs):
        return self.last_update[node_idxs]

    def clear_messages(self, nodes):
        for node in nodes:
            self.messages[node] = []

    def ensure_store(self, raw_dimension, device):
        """The device store [n_nodes, raw_dimension] (allocated empty on first use)."""
        if self.msg_raw is None or self.msg_raw.device != device or self.msg_raw.shape[1] != raw_dimension:
            self.msg_raw = torch.zeros((self.n_nodes, raw_dimension), dtype=torch.float32, device=device)
            self.msg_ts = torch.zeros(self.n_nodes, dtype=torch.float32, device=device)
            self.msg_flag = torch.zeros(self.n_nodes, dtype=torch.bool, device=device)
            self.store_is_newer = self.store_any = False

    def backup_memory(self):
        """memory.py:48-53 -> (memory, last_update, messages) clones; a fourth entry holds the device store."""
        messages_clone = {k: [(x[0].clone(), x[1].clone()) for x in v] for k, v in self.messages.items()}
        store = None
        if self.msg_raw is not None:
            store = (self.msg_raw.clone(), self.msg_ts.clone(), self.msg_flag.clone(), self.store_is_newer,
                     self.store_any)
        return self.memory.data.clone(), self.last_update.data.clone(), messages_clone, store

    def restore_memory(self, memory_backup):
        """memory.py:55-60 (a three-entry backup, as the reference's, restores without a device store)."""
        self.memory.data, self.last_update.data = memory_backup[0].clone(), memory_backup[1].clone()
        self.messages = defaultdict(list)
        for k, v in memory_backup[2].items():
            self.messages[k] = [(x[0].clone(), x[1].clone()) for x in v]
        store = memory_backup[3] if len(memory_backup) > 3 else None
        if store is None:
            self.msg_raw = self.msg_ts = self.msg_flag = None
            self.store_is_newer = self.store_any = False
        else:
            self.msg_raw, self.msg_ts, self.msg_flag = store[0].clone(), store[1].clone(), store[2].clone()
            self.store_is_newer, self.store_any = store[3], store[4]

    def detach_memory(self):
        """memory.py:62-71.  The device store never holds autograd history (it is written detached)."""
        self.memory.detach_()
        for k, v in self.messages.items():
            self.messages[k] = [(m[0].detach(), m[1]) for m in v]


class MLPMessageFunction(nn.Module):
    """message_function.py:13-25 (registered under both ``mlp`` and ``layers``, as the reference)."""

    def __init__(self, raw_message_dimension, message_dimension):
        super().__init__()
        self.mlp = self.layers = nn.Sequential(
            nn.Linear(raw_message_dimension, raw_message_dimension // 2), nn.ReLU(),
            nn.Linear(raw_message_dimension // 2, message_dimension))

    def compute_message(self, raw_messages):
        return self.mlp(raw_messages)


class IdentityMessageFunction(nn.Module):
    def compute_message(self, raw_messages):
        return raw_messages


class SequenceMemoryUpdater(nn.Module):
    """memory_updater.py:10-49 (the memory module is registered here too, as in the reference)."""

    def __init__(self, memory, message_dimension, memory_dimension, device):
        super().__init__()
        self.memory = memory
        self.layer_norm = nn.LayerNorm(memory_dimension)
        self.message_dimension = message_dimension
        self.device = device


class GRUMemoryUpdater(SequenceMemoryUpdater):
    def __init__(self, memory, message_dimension, memory_dimension, device):
        super().__init__(memory, message_dimension, memory_dimension, device)
        self.memory_updater = nn.GRUCell(input_size=message_dimension, hidden_size=memory_dimension)


class RNNMemoryUpdater(SequenceMemoryUpdater):
    def __init__(self, memory, message_dimension, memory_dimension, device):
        super().__init__(memory, message_dimension, memory_dimension, device)
        self.memory_updater = nn.RNNCell(input_size=message_dimension, hidden_size=memory_dimension)


class GraphAttentionEmbedding(nn.Module):
    """embedding_module.py:239-260 (EmbeddingModule :219-236 registers the shared tables)."""

    def __init__(self, node_features, edge_features, neighbor_finder, num_neighbor, time_encoder, n_layers,
                 n_node_features, n_edge_features, n_time_features, embedding_dimension, device, n_heads=2,
                 dropout=0.1, use_memory=True):
        super().__init__()
        self.node_features = node_features
        self.edge_features = edge_features
        self.neighbor_finder = neighbor_finder
        self.time_encoder = time_encoder
        self.n_layers = n_layers
        self.n_node_features = n_node_features
        self.n_edge_features = n_edge_features
        self.n_time_features = n_time_features
        self.dropout = dropout
        self.embedding_dimension = embedding_dimension
        self.device = device
        self.num_neighbor = num_neighbor
        self.use_memory = use_memory
        self.atten_weights_list = []
        self.n_heads = n_heads
        self.attention_models = nn.ModuleList([TemporalAttentionLayer(
            n_node_features=n_node_features, n_neighbors_features=n_node_features, n_edge_features=n_edge_features,
            time_dim=n_time_features, n_head=n_heads, dropout=dropout, output_dimension=n_node_features)
            for _ in range(n_layers)])


# ------------------------------------------------------------------ the HIP attention op (attn_op.py): TGN's own parts
def _rows_by_table_row(idx, n_rows):
    """The entries of ``idx`` grouped by the table row they name, for the reductions without atomics: a stable
    sort's permutation [len(idx)] and the segment offsets [n_rows + 1] (both int64, on idx's device; no host
    synchronisation)."""
    vals, order = torch.sort(idx.long(), stable=True)
    seg = torch.searchsorted(vals, torch.arange(n_rows + 1, dtype=torch.long, device=idx.device))
    return order.contiguous(), seg.contiguous()


class _GatherRowsFn(torch.autograd.Function):
    """tab[idx] whose backward adds the gradient rows of a table row in a fixed order (tm_tgn_rows_reduce)
    where torch's index_select backward adds with atomics.  Table row 0 is the padding node: it feeds nothing
    trainable and takes no gradient here."""

    @staticmethod
    def forward(ctx, tab, idx, err):
        ctx.save_for_backward(idx)
        ctx.err, ctx.tab_rows = err, tab.shape[0]
        return tab.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        g = g.contiguous().float()
        n, d = g.shape
        out = torch.empty((ctx.tab_rows, d), dtype=torch.float32, device=g.device)
        order, seg = _rows_by_table_row(idx, ctx.tab_rows)
        L.check(L.lib().tm_tgn_rows_reduce(L.ptr(g), n, d, L.ptr(order), n, L.ptr(seg), ctx.tab_rows, 1, L.ptr(out),
                                           L.ptr(ctx.err), L.stream_ptr(g.device)), "TGN row-gather backward")
        return out, None, None


def _gathered_table_grad(spec, desc, slot_ab, gz, tab):
    """TrainAttnFn's ``table_grad`` hook: the gradient of the gathered node table of layer 0 from the backward's
    slot_ab (tm_tgn_attn_train_dtab; no [rows*n_ngh, d_node] tensor is formed)."""
    order, seg = _rows_by_table_row(spec["node_idx"], tab.shape[0])
    d_tab = torch.empty_like(tab)
    # row 0 is the padding node: a large share of the slots, and nothing trainable behind it
    L.check(L.lib().tm_tgn_attn_train_dtab(L.C.byref(desc), L.ptr(slot_ab), L.ptr(gz), L.ptr(order), order.shape[0],
                                           L.ptr(seg), 1, L.ptr(d_tab), L.stream_ptr(gz.device)),
            "TGN gathered-table gradient")
    return d_tab


# ------------------------------------------------------------------ the model
class TGN(AL.HipTraining, nn.Module):
    """TGN/tgn.py:14-97 constructor (same arguments, submodules and initialisation order).

    ``train_on_hip()`` (attn_layer.HipTraining) opts in to the HIP training step of the stateful path
    (``forbidden_memory_update`` False): ``train()`` calls of contrast / get_node_emb / node_embeddings with
    gradients enabled run tm_tgn_attn_train_fwd / tm_tgn_attn_train_bwd, and contrast / get_node_emb advance the
    memory as tgn.py:167-191 does.  In ``eval()`` or under ``no_grad`` the stateful path needs no flag: it runs
    without dropout and advances the memory the same way."""
    _label = "TGN"
    _param_error = "TGN with memory updates: parameters must be contiguous fp32 on the HIP device (model.to(device))"

    def __init__(self, n_feat, e_feat, n_neighbors, device=None, n_layers=2, n_heads=2, dropout=0.1,
                 use_memory=True, forbidden_memory_update=False, memory_update_at_start=True, message_dimension=100,
                 memory_dimension=500, embedding_module_type="graph_attention", message_function="mlp",
                 mean_time_shift_src=0, std_time_shift_src=1, mean_time_shift_dst=0, std_time_shift_dst=1,
                 aggregator_type="last", memory_updater_type="gru", use_destination_embedding_in_message=True,
                 use_source_embedding_in_message=True, head_major_rows=True):
        super().__init__()
        if embedding_module_type != "graph_attention":
            raise NotImplementedError(f"embedding module {embedding_module_type!r}: the reference's contrast "
                                      "only runs with 'graph_attention' (embedding_update)")
        self.num_layers = n_layers
        self.ngh_finder = None
        self.device = device
        self.n_feat_th = nn.Parameter(torch.from_numpy(np.asarray(n_feat).astype(np.float32)), requires_grad=False)
        self.e_feat_th = nn.Parameter(torch.from_numpy(np.asarray(e_feat).astype(np.float32)), requires_grad=False)
        self.node_raw_features = nn.Embedding.from_pretrained(self.n_feat_th, padding_idx=0, freeze=True)
        self.edge_raw_features = nn.Embedding.from_pretrained(self.e_feat_th, padding_idx=0, freeze=True)
        self.n_node_features = self.n_feat_th.shape[1]
        self.n_nodes = self.n_feat_th.shape[0]
        self.n_edge_features = self.e_feat_th.shape[1]
        self.embedding_dimension = self.n_node_features
        self.num_neighbors = n_neighbors
        self.embedding_module_type = embedding_module_type
        self.use_destination_embedding_in_message = use_destination_embedding_in_message
        self.use_source_embedding_in_message = use_source_embedding_in_message
        self.use_memory = use_memory
        self.forbidden_memory_update = forbidden_memory_update
        self.time_encoder = TimeEncode(dimension=self.n_node_features)
        self.memory = None
        self.mean_time_shift_src, self.std_time_shift_src = mean_time_shift_src, std_time_shift_src
        self.mean_time_shift_dst, self.std_time_shift_dst = mean_time_shift_dst, std_time_shift_dst
        self.aggregator_type = aggregator_type
        self.message_function_type = message_function
        self.memory_updater_type = memory_updater_type
        if self.use_memory:
            self.memory_dimension = self.n_node_features
            self.memory_update_at_start = memory_update_at_start
            raw_message_dimension = 2 * self.memory_dimension + self.n_edge_features + self.time_encoder.dimension
            message_dimension = message_dimension if message_function != "identity" else raw_message_dimension
            self.memory = Memory(n_nodes=self.n_nodes, memory_dimension=self.memory_dimension,
                                 input_dimension=message_dimension, message_dimension=message_dimension,
                                 device=self.device)
            if aggregator_type not in ("last", "mean"):
                raise ValueError(f"Message aggregator {aggregator_type} not implemented")
            self.message_aggregator = nn.Module()   # no parameters (message_aggregator.py)
            if message_function == "mlp":
                self.message_function = MLPMessageFunction(raw_message_dimension, message_dimension)
            else:
                self.message_function = IdentityMessageFunction()
            updater = {"gru": GRUMemoryUpdater, "rnn": RNNMemoryUpdater}[memory_updater_type]
            self.memory_updater = updater(self.memory, message_dimension, self.memory_dimension, self.device)
        self.embedding_module = GraphAttentionEmbedding(
            node_features=self.node_raw_features, edge_features=self.edge_raw_features,
            neighbor_finder=self.ngh_finder, num_neighbor=self.num_neighbors, time_encoder=self.time_encoder,
            n_layers=self.num_layers, n_node_features=self.n_node_features, n_edge_features=self.n_edge_features,
            n_time_features=self.n_node_features, embedding_dimension=self.embedding_dimension, device=self.device,
            n_heads=n_heads, dropout=dropout, use_memory=self.use_memory)
        self.affinity_score = MergeLayer(self.n_node_features, self.n_node_features, self.n_node_features, 1)
        # the reference pairs attention rows with mask / explanation rows head-major through
        # .repeat(n_head, 1, 1) (embedding_module.py:74-75, :211-212); False pairs row r with row r
        self.head_major_rows = head_major_rows
        self._pack_cache = None
        self._pack_key = None

    # -------------------------------------------------------------- device pack
    def _dev(self):
        if self.device is not None and torch.device(self.device).type == "cuda":
            return L.require_device(self.device)
        p = self.n_feat_th
        return L.require_device(p.device if p.device.type == "cuda" else None)

    def _param_key(self):
        if self.use_memory and self.memory.store_is_newer:
            self.messages_to_dict()      # the stateful path moved on: the frozen path reads memory.messages
        key = [(t.data_ptr(), t._version) for t in self.parameters()]
        if self.use_memory:
            key.append(tuple((n, len(v), id(v[-1][0]) if v else 0) for n, v in sorted(self.memory.messages.items())))
        return tuple(key)

    def updated_memory(self, dev=None):
        """get_updated_memory(list(range(n_nodes)), memory.messages) (tgn.py:237-248) on the device:
        each node with stored raw messages gets one memory-updater step from its aggregated message."""
        dev = dev or self._dev()
        mem = self.memory.memory.detach().to(dev, torch.float32).clone()
        if not self.memory_update_at_start:
            return mem
        nodes = [n for n in sorted(self.memory.messages) if len(self.memory.messages[n]) > 0]
        if not nodes:
            return mem
        msgs = self.memory.messages
        if self.aggregator_type == "last":
            raw = torch.stack([msgs[n][-1][0].detach().to(dev, torch.float32) for n in nodes])
        else:
            raw = torch.stack([torch.stack([m[0].detach().to(dev, torch.float32) for m in msgs[n]]).mean(0)
                               for n in nodes])
        idx = torch.tensor(nodes, dtype=torch.long, device=dev)
        with torch.no_grad():
            fn = self.message_function
            if isinstance(fn, MLPMessageFunction):
                l0, l2 = fn.mlp[0], fn.mlp[2]
                raw = F.linear(F.relu(F.linear(raw, l0.weight.to(dev), l0.bias.to(dev))), l2.weight.to(dev),
                               l2.bias.to(dev))
            cell = self.memory_updater.memory_updater
            h = mem[idx]
            if isinstance(cell, nn.GRUCell):
                gi = F.linear(raw, cell.weight_ih.to(dev), cell.bias_ih.to(dev))
                gh = F.linear(h, cell.weight_hh.to(dev), cell.bias_hh.to(dev))
                ir, iz, inn = gi.chunk(3, 1)
                hr, hz, hn = gh.chunk(3, 1)
                r = torch.sigmoid(ir + hr)
                z = torch.sigmoid(iz + hz)
                n = torch.tanh(inn + r * hn)
                mem[idx] = (h - n) * z + n
            else:
                mem[idx] = torch.tanh(F.linear(raw, cell.weight_ih.to(dev), cell.bias_ih.to(dev))
                                      + F.linear(h, cell.weight_hh.to(dev), cell.bias_hh.to(dev)))
        return mem

    def _pack(self):
        """Device-resident tables and folded per-layer weights, rebuilt when a parameter changes."""
        dev = self._dev()
        key = (dev, self._param_key())
        if self._pack_cache is not None and self._pack_key == key:
            return self._pack_cache
        f32 = torch.float32
        with torch.no_grad():
            nf = self.n_feat_th.detach().to(dev, f32)
            tab = (self.updated_memory(dev) + nf) if self.use_memory else nf.clone()
            tw = self.time_encoder.w.weight.detach().to(dev, f32).reshape(-1).contiguous()
            tb = self.time_encoder.w.bias.detach().to(dev, f32).contiguous()
            layers = []
            for lay in self.embedding_module.attention_models[:2]:
                mh = lay.multi_head_target
                H, dk = mh.n_head, mh.d_k
                P, G = AL.fold(mh, torch.float64, dev)              # row-major: _layer multiplies by their .t() views
                layers.append(dict(
                    P=P.to(f32).contiguous(), G=G.to(f32).contiguous(), fcb=mh.fc.bias.detach().to(dev, f32),
                    lnw=mh.layer_norm.weight.detach().to(dev, f32), lnb=mh.layer_norm.bias.detach().to(dev, f32),
                    m1w=lay.merger.fc1.weight.detach().to(dev, f32), m1b=lay.merger.fc1.bias.detach().to(dev, f32),
                    m2w=lay.merger.fc2.weight.detach().to(dev, f32), m2b=lay.merger.fc2.bias.detach().to(dev, f32),
                    H=H, dk=dk, temperature=mh.temperature))
            aff = self.affinity_score
            pack = dict(dev=dev, tab=tab.contiguous(), etab=self.e_feat_th.detach().to(dev, f32).contiguous(),
                        tw=tw, tb=tb, cosb=torch.cos(tb), layers=layers,
                        a1w=aff.fc1.weight.detach().to(dev, f32), a1b=aff.fc1.bias.detach().to(dev, f32),
                        a2w=aff.fc2.weight.detach().to(dev, f32), a2b=aff.fc2.bias.detach().to(dev, f32),
                        err=torch.zeros(1, dtype=torch.int32, device=dev))
        self._pack_cache, self._pack_key = pack, key
        return pack

    # -------------------------------------------------------------- the stateful path (tgn.py:100-199)
    def _stateful(self):
        """True when contrast / get_node_emb / node_embeddings update the memory (tgn.py:167); refuses the options
        the stateful path does not restate, naming the option."""
        if not self.use_memory or self.forbidden_memory_update:
            return False
        for name, got, want in (("memory_update_at_start", self.memory_update_at_start, True),
                                ("aggregator_type", self.aggregator_type, "last"),
                                ("message_function", self.message_function_type, "mlp"),
                                ("memory_updater_type", self.memory_updater_type, "gru"),
                                ("use_source_embedding_in_message", self.use_source_embedding_in_message, True),
                                ("use_destination_embedding_in_message", self.use_destination_embedding_in_message,
                                 True)):
            if got != want:
                raise NotImplementedError(f"TGN with memory updates (forbidden_memory_update=False): {name}={got!r} "
                                          f"is not built; learn_base.py trains with {name}={want!r}")
        if len(self.embedding_module.attention_models) < 2:
            raise NotImplementedError("TGN with memory updates: n_layers < 2 (subgraphs are 2-hop: two attention "
                                      "layers run)")
        return True

    def _raw_dim(self):
        return 2 * self.memory_dimension + self.n_edge_features + self.time_encoder.dimension

    def keep_mask_shapes(self, R1, N):
        """Shapes of one step's four keep masks for R1 stacked root rows: the attention masks of layer 0 (hop-1
        rows) and layer 1 (roots), flat with the byte of (row, head, neighbour) at (row H + head) N + neighbour
        (the reference's dropped tensor [rows*n_head, 1, N]), then the masks of fc's dropout, [rows, d_query]."""
        mh = self.embedding_module.attention_models[0].multi_head_target
        H, dq = mh.n_head, 2 * self.n_node_features
        return [(R1 * N * H * N,), (R1 * H * N,), (R1 * N, dq), (R1, dq)]

    def draw_keep_masks(self, R1, N, generator=None):
        """One step's keep masks (uint8, 1 = kept with probability 1 - dropout), drawn on the device in one
        ``bernoulli_``: [attention layer 0, attention layer 1, fc layer 0, fc layer 1]."""
        return AL.draw_keep_masks(self.keep_mask_shapes(R1, N), self.embedding_module.dropout, self._dev(), generator)

    def _updated_state(self, dev):
        """get_updated_memory(all nodes, messages) (tgn.py:241-252) from the device store: M' = memory with
        GRUCell(mlp(last raw message), memory) on every node with a pending message, under autograd (memory and
        the stored messages are constants; the gradient reaches the message MLP and the GRU cell).  The cell
        runs over all nodes and ``where`` keeps the flagged rows: no host synchronisation, no compaction."""
        mem = self.memory
        if not mem.store_is_newer:
            self.messages_from_dict(dev)        # memory.messages is what counts until the first stateful step
        h = mem.memory.data
        if not mem.store_any:
            return dict(M=h)                    # nothing pending anywhere: the message MLP and the cell do not run
        l0, l2 = self.message_function.mlp[0], self.message_function.mlp[2]
        cell = self.memory_updater.memory_updater
        msg = F.linear(F.relu(F.linear(mem.msg_raw, l0.weight, l0.bias)), l2.weight, l2.bias)
        gi = F.linear(msg, cell.weight_ih, cell.bias_ih)
        gh = F.linear(h, cell.weight_hh, cell.bias_hh)
        ir, iz, inn = gi.chunk(3, 1)
        hr, hz, hn = gh.chunk(3, 1)
        r = torch.sigmoid(ir + hr)
        z = torch.sigmoid(iz + hz)
        n = torch.tanh(inn + r * hn)
        M = torch.where(mem.msg_flag.unsqueeze(1), (h - n) * z + n, h)
        return dict(M=M)

    def _layer_live(self, lay, tab, src_idx, R, N, node_idx, ngh_dense, edge_idx, edge_dense, dt, mask_node, seg,
                    akeep, fkeep, scale, tw, tb, cosb):
        """_layer on the live parameters with both dropouts of MultiHeadAttention -> [R, d_node]."""
        mh = lay.multi_head_target
        H, dk = mh.n_head, mh.d_k
        dn = self.n_node_features
        if H > 4:
            raise NotImplementedError(f"n_heads {H}: the attention kernels hold at most 4 heads")
        if tab.requires_grad:
            src = _GatherRowsFn.apply(tab, src_idx, self._train_err)
        else:
            src = tab.index_select(0, src_idx)
        query = torch.cat([src, cosb.expand(R, dn)], dim=1)                           # [R, dq]
        P, G = AL.fold(mh)
        qf = (query @ P.t()).contiguous()
        spec = AL.attn_spec("tgn", R, N, H, dk, dn, dn, mh.temperature, self.head_major_rows, seg, node_tab=tab,
                            node_idx=node_idx, edge_tab=self.e_feat_th, edge_idx=edge_idx, edge_dense=edge_dense,
                            dt=dt, mask_node=mask_node, err=self._train_err, table_grad=_gathered_table_grad)
        z = TrainAttnFn.apply(qf, ngh_dense, None if ngh_dense is not None else tab, tw, tb, spec, akeep, scale)
        # fc's dropout: embedding_module.py:84
        h = AL.mha_tail(z, query, G.t(), mh.fc.bias, mh.layer_norm.weight, mh.layer_norm.bias, fkeep, scale)
        return lay.merger(h, src)

    def _embed_live(self, x, st, explain_weights=None, edge_attr=None):
        """embedding_update_layer over tab = M' + n_feat on the live parameters (the training pair; without
        keep masks in eval() / under no_grad, where its bits are the plain kernels')."""
        if explain_weights is not None:
            raise NotImplementedError("TGN with memory updates: explain_weights (the explainer runs on the frozen "
                                      "model, forbidden_memory_update=True)")
        train = self.training and torch.is_grad_enabled()
        if train and not self._train_on_hip:
            raise NotImplementedError("TGN in train() mode with memory updates: call model.train_on_hip() first "
                                      "(the HIP training step is opt-in; eval() / no_grad need no flag)")
        R1, N, seg1 = x["R"], x["N"], x["seg"]
        p = float(self.embedding_module.dropout) if train else 0.0
        keep, scale = AL.step_keep_masks(
            getattr(self, "tgn_keep_masks", None) if train else None, self.keep_mask_shapes(R1, N), p, st["M"].device,
            "TGN.tgn_keep_masks: expected draw_keep_masks(R1, N)'s four uint8 masks on the device")
        tab = (st["M"] + self.n_feat_th).contiguous()
        te = self.time_encoder
        tw, tb = te.w.weight.view(-1), te.w.bias
        cosb = torch.cos(tb)
        lay0, lay1 = self.embedding_module.attention_models[0], self.embedding_module.attention_models[1]
        # layer 0: hop-1 nodes attend over their hop-2 neighbours, keys gathered from tab
        y0 = self._layer_live(lay0, tab, x["n1l"], R1 * N, N, x["n2"], None, x["e2"], x["ed2"], x["dt2"], x["n2"],
                              seg1 * N, keep[0], keep[2], scale, tw, tb, cosb)
        # layer 1: roots attend over the hop-1 embeddings
        y1 = self._layer_live(lay1, tab, x["n0"], R1, N, None, y0.contiguous(), x["e1"], x["ed1"], x["dt1"],
                              x["n1"], seg1, keep[1], keep[3], scale, tw, tb, cosb)
        self._tgn_train_key = (R1, N, keep[0] is not None)   # marker: the stateful path ran
        return y1

    def _stateful_embed(self, x, src_idx, tgt_idx, cut_time, e_idx, explain_weights=None, edge_attr=None):
        """get_node_emb with memory updates (tgn.py:123-196): embeddings over the updated memory, then the state
        moves on with this step's values (no gradient flows into the stored state)."""
        dev = self._live_state(self._dev())
        st = self._updated_state(dev)
        emb = self._embed_live(x, st, explain_weights, edge_attr)
        if len(src_idx) > 0:
            with torch.no_grad():
                self._advance_state(st["M"].detach(), emb.detach(), src_idx, tgt_idx, cut_time, e_idx, dev)
        return emb

    def _advance_state(self, M, emb, src_idx, tgt_idx, cut_time, e_idx, dev):
        """tgn.py:167-191 on the device, without a loop over events or nodes and without a host synchronisation:
        persist the positives' updated memory and clear their messages, then store this batch's raw messages.
        Of a node's messages the ``last`` aggregator reads the last one: source-role messages are appended before
        destination-role ones, each in batch order, so the winner is the entry with the largest index in
        [src | dst] -- read off a stable sort, never off a scatter with duplicate indices."""
        mem = self.memory
        if e_idx is None:
            raise ValueError("TGN with memory updates: e_idx is needed for the raw messages")
        B, n = len(src_idx), self.n_nodes
        src = as_dev(src_idx, dev, torch.long).reshape(-1)
        dst = as_dev(tgt_idx, dev, torch.long).reshape(-1)
        pos = torch.cat([src, dst])
        vals, order = torch.sort(pos, stable=True)
        ar = torch.arange(n, dtype=torch.long, device=dev)
        hi = torch.searchsorted(vals, ar, right=True)
        is_pos = hi > torch.searchsorted(vals, ar)
        sel = order[(hi - 1).clamp_min(0)]                  # a positive's last entry in [src | dst]
        # update_memory(positives): only positives with a pending message change
        apply = is_pos & mem.msg_flag
        mem.memory.data = torch.where(apply.unsqueeze(1), M, mem.memory.data)
        mem.last_update.data = torch.where(apply, mem.msg_ts, mem.last_update.data)
        # get_raw_messages (:254-278) with the just updated last_update and ts cast to fp32
        ts = as_dev(cut_time, dev, torch.float64).reshape(-1)[:B].float()
        lu = mem.last_update.data
        ef = self.e_feat_th.index_select(0, as_dev(e_idx, dev, torch.long).reshape(-1))
        w64, b64 = self.time_encoder.w.weight.detach().view(1, -1).double(), self.time_encoder.w.bias.detach().double()

        def tenc(delta):
            # Linear(1, d) rounds dt*w + b once (an fma): the exact fp64 product and sum, rounded to fp32
            return torch.cos((delta.double().unsqueeze(1) * w64 + b64).float())
        s_emb, d_emb = emb[:B], emb[B:2 * B]
        msgs = torch.cat([torch.cat([s_emb, d_emb, ef, tenc(ts - lu[src])], dim=1),
                          torch.cat([d_emb, s_emb, ef, tenc(ts - lu[dst])], dim=1)])
        ts2 = torch.cat([ts, ts])
        mem.msg_raw = torch.where(is_pos.unsqueeze(1), msgs.index_select(0, sel), mem.msg_raw)
        mem.msg_ts = torch.where(is_pos, ts2[sel], mem.msg_ts)
        mem.msg_flag = mem.msg_flag | is_pos
        mem.store_is_newer = mem.store_any = True
        mem.messages = defaultdict(list)       # stale from here on; messages_to_dict() rebuilds it

    def messages_from_dict(self, dev=None):
        """memory.messages -> the device store: of every node's list the last (raw message, timestamp)."""
        if self.aggregator_type != "last":
            raise NotImplementedError(f"aggregator_type {self.aggregator_type!r}: the device store keeps a node's "
                                      "last message only ('mean' reads them all)")
        dev = dev or self._dev()
        mem = self.memory
        mem.ensure_store(self._raw_dim(), dev)
        mem.msg_flag = torch.zeros_like(mem.msg_flag)
        nodes = [int(k) for k, v in mem.messages.items() if len(v) > 0]
        if nodes:
            last = [mem.messages[k][-1] for k in nodes]
            idx = torch.tensor(nodes, dtype=torch.long, device=dev)
            raw = torch.stack([m[0].detach().to(dev, torch.float32) for m in last])
            ts = torch.stack([torch.as_tensor(m[1]).detach().to(dev, torch.float32).reshape(()) for m in last])
            mem.msg_raw = mem.msg_raw.index_copy(0, idx, raw)
            mem.msg_ts = mem.msg_ts.index_copy(0, idx, ts)
            mem.msg_flag = mem.msg_flag.index_fill(0, idx, True)
        mem.store_is_newer, mem.store_any = False, bool(nodes)
        return self

    def pending_messages(self):
        """{"nodes" [K] int64, "raw" [K, raw_dim], "ts" [K]}: the nodes with a pending message, ascending, and
        their last raw message and its timestamp (synchronises)."""
        mem = self.memory
        if not mem.store_is_newer:
            self.messages_from_dict()
        nodes = torch.nonzero(mem.msg_flag).reshape(-1)
        return {"nodes": nodes, "raw": mem.msg_raw.index_select(0, nodes), "ts": mem.msg_ts.index_select(0, nodes)}

    def load_pending_messages(self, saved, dev=None):
        """pending_messages()'s dict (as learn_base saves it next to the state_dict) -> the device store."""
        dev = dev or self._dev()
        mem = self.memory
        mem.ensure_store(self._raw_dim(), dev)
        idx = saved["nodes"].to(dev, torch.long)
        mem.msg_raw = torch.zeros_like(mem.msg_raw).index_copy(0, idx, saved["raw"].to(dev, torch.float32))
        mem.msg_ts = torch.zeros_like(mem.msg_ts).index_copy(0, idx, saved["ts"].to(dev, torch.float32))
        mem.msg_flag = torch.zeros_like(mem.msg_flag).index_fill(0, idx, True)
        mem.store_is_newer, mem.store_any = True, idx.numel() > 0
        mem.messages = defaultdict(list)
        return self

    def messages_to_dict(self):
        """The device store -> memory.messages (what the frozen path and the reference's methods read): one
        (raw message, timestamp) entry per node with a pending message."""
        mem = self.memory
        if not mem.store_is_newer:
            return self                          # memory.messages is what counts already
        out = defaultdict(list)
        if mem.msg_flag is not None:
            nodes = torch.nonzero(mem.msg_flag).reshape(-1)
            raw, ts = mem.msg_raw.index_select(0, nodes), mem.msg_ts.index_select(0, nodes)
            for i, k in enumerate(nodes.tolist()):
                out[k] = [(raw[i], ts[i])]
        mem.messages = out
        mem.store_is_newer = False
        return self

    # -------------------------------------------------------------- forward pieces
    def _layer(self, pk, li, src_feat, R, N, node_idx, ngh_dense, edge_idx, edge_dense, dt, mask_node, ew, seg=0,
               cache=None, tap=None):
        """One TemporalAttentionLayer over R source rows (embedding_module.py:181-216).  ``cache`` (the
        prepared inputs' dict): the query and its folded projection depend on the source rows and the frozen
        weights only, so the training step's two contrasts of one batch (temp_exp_main.py:597, :611) compute
        them once.  ``tap`` (a list, ``attention_weights``): the layer's attention probabilities and their head
        mean are appended to it, from one more launch on the forward's descriptor."""
        lw = pk["layers"][li]
        H, dk = lw["H"], lw["dk"]
        dn = self.n_node_features
        key = ("qf", li, id(pk))
        hit = cache.get(key) if cache is not None else None
        if hit is not None and hit[0] is pk:
            query, qf = hit[1], hit[2]
        else:
            query = torch.cat([src_feat(), pk["cosb"].expand(R, dn)], dim=1)    # [R, dq]
            qf = (query @ lw["P"].t()).contiguous()                            # [R, H*dk]
            if cache is not None:
                cache[key] = (pk, query, qf)
        src_feat = query[:, :dn]
        spec = AL.attn_spec("tgn", R, N, H, dk, dn, dn, lw["temperature"], self.head_major_rows, seg,
                            node_tab=pk["tab"], node_idx=node_idx, edge_tab=pk["etab"], edge_idx=edge_idx,
                            edge_dense=edge_dense, dt=dt, time_w=pk["tw"], time_b=pk["tb"], mask_node=mask_node,
                            err=pk["err"])
        if tap is not None:
            tap.append(attn_probs(spec, qf, ngh_dense))
        z = AttnFn.apply(qf, ngh_dense, ew, spec)
        h = AL.mha_tail(z, query, lw["G"].t(), lw["fcb"], lw["lnw"], lw["lnb"])
        x = torch.cat([h, src_feat], dim=1)
        return F.linear(F.relu(F.linear(x, lw["m1w"], lw["m1b"])), lw["m2w"], lw["m2b"])

    def node_embeddings(self, nodes, eids, times, cut_time, explain_weights=None, edge_attr=None, n_segments=1,
                        prepared=None, tap=None):
        """embedding_update(_attr) + embedding_update_layer (embedding_module.py:314-393) for
        nodes = [n0 [R1], n1 [R1,N], n2 [R1,N^2]], eids/times = [hop1, hop2] -> [R1, d].
        n_segments > 1 stacks independent contrast batches (R1 = n_segments * 3B rows): every row
        gives the same result as in its own call (the head-major pairing stays inside its batch).
        ``prepared``: the output of ``_prep_inputs`` for these inputs (built once when the same
        subgraphs go through several contrasts, as the training step's two do).  ``tap``: ``_layer``'s, filled
        with layer 0's pair and then layer 1's (the frozen model only)."""
        if self._stateful():
            if tap is not None:
                raise NotImplementedError("TGN attention weights with memory updates (forbidden_memory_update="
                                          "False): the frozen model's layers are tapped, as the explainer reads it")
            x = prepared if prepared is not None else self._prep_inputs(nodes, eids, times, cut_time, edge_attr,
                                                                        n_segments)
            # no events here: the embeddings over the updated memory, the state left as it is
            return self._embed_live(x, self._updated_state(self._live_state(self._dev())), explain_weights, edge_attr)
        pk = self._pack()
        x = prepared if prepared is not None else self._prep_inputs(nodes, eids, times, cut_time, edge_attr, n_segments)
        R1, N, seg1 = x["R"], x["N"], x["seg"]
        dev = pk["dev"]
        ew1 = ew2 = None
        if explain_weights is not None:
            ew1 = explain_weights[0].to(dev, torch.float32).reshape(R1, N).contiguous()
            ew2 = explain_weights[1].to(dev, torch.float32).reshape(R1 * N, N).contiguous()
        tab = pk["tab"]
        # layer 0 (attention_models[0]): hop-1 nodes attend over their hop-2 neighbours
        cache = x if prepared is not None else None
        y0 = self._layer(pk, 0, lambda: tab[x["n1l"]], R1 * N, N, x["n2"], None, x["e2"], x["ed2"], x["dt2"],
                         x["n2"], ew2, seg1 * N, cache, tap)
        # layer 1 (attention_models[1]): roots attend over the hop-1 embeddings
        y1 = self._layer(pk, 1, lambda: tab[x["n0"]], R1, N, None, y0.contiguous(), x["e1"], x["ed1"], x["dt1"],
                         x["n1"], ew1, seg1, cache, tap)
        return y1

    def _prep_inputs(self, nodes, eids, times, cut_time, edge_attr=None, n_segments=1):
        """node_embeddings' index, time-offset and edge-attribute tensors (retrieve_time_features etc.)."""
        x = AL.prep_inputs(self._dev(), nodes, eids, times, cut_time, n_segments, sides=3, lone_seg_rows=False,
                           edge_attr=edge_attr)
        x["n1l"] = x["n1"].long()          # the hop-1 nodes as layer 0's source rows (an index into the table)
        return x

    # -------------------------------------------------------------- reference API
    def get_node_emb(self, src_idx, tgt_idx, bgd_idx, cut_time, e_idx, subgraph_src, subgraph_tgt, subgraph_bgd,
                     explain_weights=None, edge_attr=None, prepared=None):
        """tgn.py:99-199 -> (source, destination, negative) embeddings [B, d] each."""
        B = len(src_idx)
        stateful = self._stateful()
        if prepared is None:
            prepared = self.prepare_contrast(src_idx, tgt_idx, bgd_idx, cut_time, subgraph_src, subgraph_tgt,
                                             subgraph_bgd, edge_attr)
        if stateful:
            emb = self._stateful_embed(prepared, src_idx, tgt_idx, cut_time, e_idx, explain_weights, edge_attr)
        else:
            emb = self.node_embeddings(None, None, None, None, explain_weights, edge_attr, prepared=prepared)
        # split (one backward: a cat of the three gradients) rather than three slices (a zero-filled full-size
        # gradient, a copy and an add each)
        return tuple(emb.split(B)) if B > 0 else (emb[:0], emb[:0], emb[:0])

    def prepare_contrast(self, src_idx, tgt_idx, bgd_idx, cut_time, subgraph_src, subgraph_tgt, subgraph_bgd,
                         edge_attr=None):
        """The inputs contrast derives from its batch (the three sides' roots and subgraphs
        concatenated, time offsets), built once: the training step's two contrasts of the same batch
        (without and with explanation weights, temp_exp_main.py:597, :611) share them."""
        roots, nodes, eids, times = AL.stack_sides(self._dev(), (src_idx, tgt_idx, bgd_idx),
                                                   (subgraph_src, subgraph_tgt, subgraph_bgd), eids=edge_attr is None)
        return self._prep_inputs([roots] + nodes, eids, times, cut_time, edge_attr)

    def affinity(self, x1, x2):
        return AL.affinity(self._pack(), x1, x2)

    def attention_weights(self, src_idx, tgt_idx, bgd_idx, cut_time, subgraph_src, subgraph_tgt, subgraph_bgd,
                          prepared=None, head_mean=False):
        """The attention probabilities of the contrast without explanation weights, as the reference's attention
        modules return them: (hop-1 [3B, H, N], hop-2 [3B N, H, N]) fp32 device tensors, rows in the order src, tgt,
        bgd.  Hop-1 is layer 1, the roots over the hop-1 embeddings; hop-2 is layer 0, the hop-1 nodes over their
        hop-2 neighbours.  The frozen embedding pass runs once (the hop-1 keys are layer 0's output) with one
        ``tm_tgn_attn_probs`` launch per layer on the forward's descriptor.  A padded slot carries whatever the
        softmax gives it (a fully padded row is uniform); ``baselines.attention_explanation`` zeroes them.
        ``head_mean``: the means over the heads instead, (hop-1 [3B, N], hop-2 [3B N, N]).  ``prepared``:
        prepare_contrast's output for these inputs.  No gradient.  A stateful TGN (forbidden_memory_update=False)
        raises NotImplementedError: the explainer reads the frozen model."""
        if self._stateful():
            raise NotImplementedError("TGN.attention_weights with memory updates (forbidden_memory_update=False): "
                                      "the frozen model's layers are tapped, as the explainer reads it")
        with torch.no_grad():
            if prepared is None:
                prepared = self.prepare_contrast(src_idx, tgt_idx, bgd_idx, cut_time, subgraph_src, subgraph_tgt,
                                                 subgraph_bgd)
            tap = []
            self.node_embeddings(None, None, None, None, prepared=prepared, tap=tap)
        (p2, m2), (p1, m1) = tap
        return (m1, m2) if head_mean else (p1, p2)

    def contrast(self, src_idx, tgt_idx, bgd_idx, cut_time, e_idx, subgraph_src, subgraph_tgt, subgraph_bgd,
                 explain_weights=None, edge_attr=None, prepared=None):
        """tgn.py:201-218 -> (pos_score [B,1], neg_score [B,1]).  ``prepared``: prepare_contrast's
        output for these same inputs (optional, shared by several contrasts of one batch)."""
        B = len(src_idx)
        stateful = self._stateful()
        if prepared is None:
            prepared = self.prepare_contrast(src_idx, tgt_idx, bgd_idx, cut_time, subgraph_src, subgraph_tgt,
                                             subgraph_bgd, edge_attr)
        if stateful:
            emb = self._stateful_embed(prepared, src_idx, tgt_idx, cut_time, e_idx, explain_weights, edge_attr)
        else:
            emb = self.node_embeddings(None, None, None, None, explain_weights, edge_attr, prepared=prepared)
        if B == 0:
            return emb[:0, :1], emb[:0, :1]
        # get_node_emb's (s, d, n) as two pieces of one split: [d; n] is emb's tail (no copy), and the backward
        # is one cat instead of a zero-filled full-size gradient, a copy and an add per slice
        s, dn = emb.split([B, 2 * B])
        if stateful:
            score = self.affinity_score(torch.cat([s, s], dim=0), dn).squeeze(dim=0)      # the live parameters
        else:
            score = self.affinity(torch.cat([s, s], dim=0), dn).squeeze(dim=0)
        return tuple(score.split(B))

    def retrieve_edge_features(self, subgraph_src, subgraph_tgt, subgraph_bgd):
        """tgn.py:220-228: [E_feat[hop-1 eids], E_feat[hop-2 eids]] for the three sides."""
        dev = self._dev()
        et = self._pack()["etab"]
        out = []
        for h in (0, 1):
            idx = torch.cat([as_dev(sg[1][h], dev, torch.long) for sg in (subgraph_src, subgraph_tgt, subgraph_bgd)])
            out.append(et[idx])
        return out

    def set_neighbor_sampler(self, neighbor_finder):
        self.embedding_module.neighbor_sampler = neighbor_finder

    def grab_subgraph(self, src_idx_l, cut_time_l):
        """tgn.py:283-285."""
        return self.embedding_module.neighbor_sampler.find_k_hop(2, src_idx_l, cut_time_l,
                                                                 num_neighbors=self.num_neighbors, e_idx_l=None)

    def embedding_temperature(self, layer=0):
        return self.embedding_module.attention_models[layer].multi_head_target.temperature


def node_records_cat(subgraph, dev):
    """[hop-1 | hop-2] node records of one side as one int32 device tensor [B, N + N^2]."""
    return torch.cat([as_dev(subgraph[0][0], dev, torch.int32), as_dev(subgraph[0][1], dev, torch.int32)], dim=1)


__all__ = ["TGN", "TimeEncode", "MergeLayer", "TemporalAttentionLayer", "MultiHeadAttention", "Memory",
           "node_records_cat"]
