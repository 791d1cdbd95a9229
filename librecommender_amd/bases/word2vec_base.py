"""`Word2VecBase` (`libreco/bases/gensim_base.py`, there `GensimBase`): the models whose training the reference hands to
`gensim.Word2Vec` on CPU threads, Item2Vec and DeepWalk.  Here the whole of it runs on the device (csrc/word2vec.hip): the
corpus of an epoch (random walks, frequent-word subsampling, the shrinking context window), the targets of every pair
(the predicted word, 5 draws from the count^0.75 table, the Huffman path) and the updates of the input table `syn0` and the
output table `syn1`.  There is no CPU engine and gensim is no dependency.

word2vec walks the pairs one after the other; here an epoch's pairs are cut into windows of `batch_size` pairs (DESIGN.md
§7.9), as BPR's engine does with its triples (§7.4): every f and g of a window comes from the tables as they stood when the
window began, and each touched row then takes its sum in ascending sample order.  Two runs give the same bits.

Deliberate differences from gensim: the window; the counter-based generator (every draw is a function of (seed, position));
the exact sigmoid instead of the 1000-entry table; the vocabulary indexed by the item's inner id; the step size per pair
instead of per job; `n_threads` accepted and ignored.  Nothing here was compared with gensim's output.
"""
from __future__ import annotations

import abc
import heapq

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..evaluation.evaluate import print_metrics
from ..layers.row_adam import NamedTables
from ..utils.misc import time_block
from ..utils.validate import check_fitting
from .base import hip_device
from .embed_base import EmbedBase

SAMPLE = 1e-3                    # gensim's default `sample`
CHUNK_PAIRS = 1 << 20            # pairs whose targets are built by one call (a whole number of windows)
# `batch_size` is capped (profiles/word2vec.md): summed stale updates at alpha 0.025 diverge when the window is large against
# the rows it touches.  Negatives: 8 pairs per item of the vocabulary was inside the run-to-run spread of window 1, 33 per item
# diverged.  With hierarchical softmax the root of the tree is a target of every pair whatever the vocabulary: 1,024 pairs held,
# 4,096 diverged.
MAX_WINDOW_PER_ITEM = 8
MAX_WINDOW_HS = 1024


def keep_thresholds(counts: np.ndarray, sample: float = SAMPLE) -> np.ndarray:
    """floor(2^32 * min(1, (sqrt(c / (sample T)) + 1) * sample T / c)) per word (int64), 0 for a word that never occurs."""
    c = counts.astype(np.float64)
    thr = sample * float(counts.sum())
    out = np.zeros(len(counts), dtype=np.int64)
    nz = counts > 0
    out[nz] = np.floor(np.minimum(1.0, (np.sqrt(c[nz] / thr) + 1.0) * thr / c[nz]) * 4294967296.0).astype(np.int64)
    return out


def negative_table(counts: np.ndarray) -> np.ndarray:
    """The cumulative count^0.75 table scaled to 2^32 (int64 [n_items]): a draw r picks the first word with cum > r, so a
    word that never occurs is never drawn."""
    w = np.where(counts > 0, counts.astype(np.float64) ** 0.75, 0.0)
    cs = np.cumsum(w)
    if len(cs) == 0 or cs[-1] <= 0:
        return np.zeros(len(counts), dtype=np.int64)
    cum = np.floor(cs / cs[-1] * 4294967296.0).astype(np.int64)
    cum[np.flatnonzero(counts > 0)[-1]:] = 1 << 32
    return cum


def huffman_csr(counts: np.ndarray):
    """The Huffman tree over the words that occur, built with `heapq` over (count, index); the k-th merge gets index
    n_items + k (its row in `syn1`), its first-popped child code 0 and the other code 1.  -> int32 CSR per word of the inner
    nodes from the root down and the codes: (ptr [n_items + 1], nodes, codes)."""
    n = len(counts)
    heap = [(int(c), i) for i, c in enumerate(counts) if c > 0]
    heapq.heapify(heap)
    parent = np.full(2 * n, -1, dtype=np.int64)
    code = np.zeros(2 * n, dtype=np.int32)
    k = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        parent[a[1]], parent[b[1]], code[b[1]] = n + k, n + k, 1
        heapq.heappush(heap, (a[0] + b[0], n + k))
        k += 1
    ptr, nodes, codes = np.zeros(n + 1, dtype=np.int32), [], []
    for w in range(n):
        path, x = [], w
        while parent[x] >= 0:
            path.append((parent[x], code[x]))
            x = parent[x]
        nodes.extend(p for p, _ in reversed(path))
        codes.extend(c for _, c in reversed(path))
        ptr[w + 1] = len(nodes)
    return ptr, np.asarray(nodes, dtype=np.int32), np.asarray(codes, dtype=np.int32)


def flatten_lists(lists):
    """-> (tokens int32 [T], sptr int64 [S + 1]) of a list of id lists."""
    sptr = np.zeros(len(lists) + 1, dtype=np.int64)
    if len(lists):
        sptr[1:] = np.cumsum([len(s) for s in lists])
    parts = [np.asarray(s, dtype=np.int32).reshape(-1) for s in lists if len(s)]
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)), sptr


class Word2VecBase(EmbedBase):
    use_hs = False               # hierarchical softmax next to the negatives (DeepWalk)

    def __init__(self, task, data_info, embed_size=16, norm_embed=False, window_size=5, n_epochs=5, n_threads=0, seed=42,
                 lower_upper_bound=None, batch_size=256, device="cuda"):
        super().__init__(task, data_info, embed_size, lower_upper_bound)
        if not isinstance(embed_size, (int, np.integer)) or not 1 <= embed_size <= 256:
            raise ValueError(f"{type(self).__name__} supports `embed_size` from 1 to 256 (a row is held in one wave's "
                             f"registers), got {embed_size}")
        if not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError("`batch_size` (the window, in pairs) must be at least 1")
        self.norm_embed = norm_embed
        self.window_size = 5 if not window_size else window_size
        self.n_epochs = n_epochs
        self.n_threads = n_threads             # accepted and ignored
        self.seed = seed
        self.batch_size, self._device_arg = int(batch_size), device
        self.syn0 = self.syn1 = None           # [n_items, D], [n_items (+ n_items - 1 inner nodes with `use_hs`), D]
        self.counts = None                     # int64 [n_items], host: occurrences in pass 0 of the corpus
        self._epochs_done = 0
        self.last_epoch_loss = None            # mean loss per pair of the last epoch (verbose runs only)
        self.last_epoch_pairs = None           # (input ids, predicted ids, raw centre positions) of the last epoch

    # ---- corpus -----------------------------------------------------------------------------------------------------
    @abc.abstractmethod
    def corpus(self, pass_no):
        """-> (tokens int32 [T], sptr int64 [S + 1]) on the device: the sentences of pass `pass_no` (0 gives the counts)."""

    def window_pairs(self):
        """The window actually used: `batch_size`, capped at MAX_WINDOW_PER_ITEM pairs per item and, with hierarchical
        softmax, at MAX_WINDOW_HS pairs."""
        W = min(self.batch_size, MAX_WINDOW_PER_ITEM * self.n_items)
        return max(1, min(W, MAX_WINDOW_HS) if self.use_hs else W)

    # ---- model ------------------------------------------------------------------------------------------------------
    def initial_tables(self):
        rng = np.random.default_rng(self.seed)
        D = self.embed_size
        syn0 = ((rng.random((self.n_items, D), dtype=np.float32) - 0.5) / D).astype(np.float32)
        rows1 = self.n_items + (max(self.n_items - 1, 0) if self.use_hs else 0)
        return syn0, np.zeros((rows1, D), dtype=np.float32)

    def build_model(self):
        self.device = hip_device(self._device_arg)
        syn0, syn1 = self.initial_tables()
        self.syn0, self.syn1 = torch.from_numpy(syn0).to(self.device), torch.from_numpy(syn1).to(self.device)
        self._prepare_corpus()
        tokens, _ = self.corpus(0)
        t = tokens[(tokens >= 0) & (tokens < self.n_items)].long()
        self.counts = torch.bincount(t, minlength=self.n_items).cpu().numpy().astype(np.int64)
        self._upload_vocabulary()

    def _prepare_corpus(self):
        pass

    def _upload_vocabulary(self):
        dev = self.device
        self.total_words = int(self.counts.sum())
        self._thr = torch.from_numpy(keep_thresholds(self.counts)).to(dev)
        self._cum = torch.from_numpy(negative_table(self.counts)).to(dev)
        self._hs = tuple(torch.from_numpy(a).to(dev) for a in huffman_csr(self.counts)) if self.use_hs else None

    def train_on_batch(self, batch):
        raise NotImplementedError(f"{self.model_name} trains by epochs of windows on the device, not by collated batches")

    # ---- the engine -------------------------------------------------------------------------------------------------
    def epoch_pairs(self, epoch):
        """The pair list of an epoch on the device: keep flags, compaction (torch ops), count / scan / emit."""
        tokens, sptr = self.corpus(epoch)
        keep = ops.w2v_keep(tokens, self._thr, self.seed, epoch)
        craw = torch.nonzero(keep).view(-1).to(torch.int32)
        sent = torch.repeat_interleave(torch.arange(sptr.numel() - 1, device=self.device, dtype=torch.int32),
                                       sptr[1:] - sptr[:-1])
        idx = craw.long()
        pre = F.pad(torch.cumsum(keep, 0, dtype=torch.int64), (1, 0))
        return ops.w2v_pairs(tokens[idx].contiguous(), craw, sent[idx].contiguous(), pre[sptr].contiguous(),
                             self.window_size, self.seed, epoch)

    def engine_window(self, ins, centre, tg, s0, s1, a, b, pos0, inv_total, bufs, want_loss):
        """One window (pairs a .. b of the chunk, target slots s0 .. s1): score against the tables as they stand, then the
        ordered update of the touched output rows (which reads the input rows, still untouched) and of the touched input
        rows (which reads only the stash)."""
        _, stash, loss = ops.w2v_score(self.syn0, self.syn1, ins[a:b], centre[a:b], tg["offs"][a:b + 1], tg["rows"], tg["labels"],
                                       pos0, inv_total, g=bufs["g"], stash=bufs["stash"], want_loss=want_loss)
        seg_o = bufs["seg_out"].build(tg["rows"][s0:s1])
        seg_i = bufs["seg_in"].build(ins[a:b])
        ops.w2v_out_update(self.syn1, seg_o, self.syn0, bufs["g"][s0:s1], tg["slot_in"][s0:s1])
        ops.w2v_out_update(self.syn0, seg_i, stash)
        return loss

    def engine_epoch(self, epoch, want_loss=False):
        ins, pred, centre = self.epoch_pairs(epoch)
        self.last_epoch_pairs = (ins, pred, centre)
        n, W = ins.numel(), self.window_pairs()
        if n == 0 or self.total_words == 0:
            return 0, None
        W = min(W, n)
        chunk = max(W, CHUNK_PAIRS // W * W)
        pos0, inv_total = float((epoch - 1) * self.total_words), 1.0 / (self.n_epochs * self.total_words)
        stash = torch.empty((W, self.embed_size), dtype=torch.float32, device=self.device)
        loss_sum = torch.zeros((), dtype=torch.float64, device=self.device) if want_loss else None
        for c0 in range(0, n, chunk):
            c1 = min(c0 + chunk, n)
            tg = ops.w2v_targets(ins[c0:c1], pred[c0:c1], self._cum, self.seed, epoch, pair_base=c0, hs=self._hs)
            starts = list(range(0, c1 - c0, W)) + [c1 - c0]
            if self._hs is None:
                slot = [(ops.W2V_NEGATIVES + 1) * a for a in starts]
            else:                                    # the windows' slot ranges: one read-back per chunk
                slot = tg["offs"][torch.tensor(starts, device=self.device)].cpu().tolist()
            widest = max(s1 - s0 for s0, s1 in zip(slot[:-1], slot[1:]))
            bufs = {"g": torch.empty(max(slot[-1], 1), dtype=torch.float32, device=self.device), "stash": stash,
                    "seg_out": ops.SegmentBuilder(max(widest, 1), self.syn1.shape[0], self.device),
                    "seg_in": ops.SegmentBuilder(W, self.n_items, self.device)}
            ic, cc = ins[c0:c1], centre[c0:c1]
            for w, a in enumerate(starts[:-1]):
                loss = self.engine_window(ic, cc, tg, slot[w], slot[w + 1], a, starts[w + 1], pos0, inv_total, bufs, want_loss)
                if want_loss:
                    loss_sum += loss.sum(dtype=torch.float64)
        return n, loss_sum

    def fit(self, train_data, neg_sampling, verbose=1, shuffle=True, eval_data=None, metrics=None, k=10,
            eval_batch_size=8192, eval_user_num=None, **kwargs):
        check_fitting(self, train_data, eval_data, neg_sampling, k)
        from .. import distributed as D

        if D.active() is not None:
            raise RuntimeError(f"{self.model_name}: multi-GPU `fit` (torch.distributed is initialised with more than one "
                               "rank) is implemented for TwoTower, LightGCN, FM / DeepFM with plain sparse columns and DIN "
                               "on pure ids; run this model in a single process")
        self.show_start_time()
        if not self.model_built:
            self.build_model()
            self.model_built = True
        for epoch in range(1, self.n_epochs + 1):
            with time_block(f"Epoch {epoch}", verbose):
                n, loss_sum = self.engine_epoch(epoch, want_loss=verbose > 0)
                torch.cuda.synchronize(self.device)
            self._epochs_done = epoch
            if verbose > 0 and loss_sum is not None:
                self.last_epoch_loss = float(loss_sum) / max(n, 1)
                print(f"\t train_loss: {self.last_epoch_loss:.4f} ({n} pairs)")
        self.after_fit()
        if verbose > 1:
            print_metrics(model=self, neg_sampling=neg_sampling, eval_data=eval_data, metrics=metrics,
                          eval_batch_size=eval_batch_size, k=k, sample_user_num=eval_user_num, seed=self.seed)
            print("=" * 30)

    # ---- export -----------------------------------------------------------------------------------------------------
    def _consumed_mean_csr(self):
        lists = [self.user_consumed.get(u, ()) for u in range(self.n_users)]
        idx, ptr = flatten_lists(lists)
        lens = np.diff(ptr)
        val = np.repeat(1.0 / np.maximum(lens, 1), lens).astype(np.float32)
        return tuple(torch.from_numpy(a).to(self.device) for a in (ptr, idx, val))

    def set_embeddings(self):
        """`gensim_base.py:96-108`: the item rows are `syn0` (l2-normalised with `norm_embed`), a user's row the mean of the
        item rows over the consumed list, computed on the device from the consumed CSR."""
        items = F.normalize(self.syn0, dim=1, eps=1e-12) if self.norm_embed else self.syn0.clone()
        ptr, idx, val = self._consumed_mean_csr()
        self.item_embeds = items.contiguous()
        self.user_embeds = ops.spmm_csr(ptr, idx, val, self.item_embeds)

    # ---- persistence ------------------------------------------------------------------------------------------------
    def variables_np(self):
        return {"w2v/syn0": self.syn0.cpu().numpy(), "w2v/syn1": self.syn1.cpu().numpy(), "w2v/counts": np.asarray(self.counts)}

    def optimizer_arrays(self):
        return {"opt::epochs": np.asarray(self._epochs_done, dtype=np.int64)}

    def load_variables_np(self, arrays):
        with torch.no_grad():
            if "w2v/syn0" in arrays:
                self.syn0.copy_(torch.from_numpy(arrays["w2v/syn0"]))
                self.syn1.copy_(torch.from_numpy(arrays["w2v/syn1"]))
            if "w2v/counts" in arrays and len(arrays["w2v/counts"]) == self.n_items:
                self.counts = arrays["w2v/counts"].astype(np.int64)
                self._upload_vocabulary()

    def rebuild_model(self, path, model_name):
        """Retraining on merged data (`gensim_base.py:135-151`): the freshly built, larger model takes over the saved rows by
        id; the inner-node rows of the Huffman tree are taken over by index.  New items keep their fresh draws; counts, the
        negative table and the tree come from the new corpus."""
        arrays, old = self._begin_rebuild(path, model_name)
        n_old, n_new = int(old.n_items), self.n_items
        saved1 = arrays["w2v/syn1"]
        tables = {"w2v/syn0": self.syn0, "w2v/syn1neg": self.syn1[:n_new]}
        taken = {"w2v/syn0": arrays["w2v/syn0"], "w2v/syn1neg": saved1[:n_old]}
        rows = {"w2v/syn0": n_old, "w2v/syn1neg": n_old}
        if self.use_hs and saved1.shape[0] > n_old:
            tables["w2v/syn1hs"], taken["w2v/syn1hs"] = self.syn1[n_new:], saved1[n_old:]
            rows["w2v/syn1hs"] = min(saved1.shape[0] - n_old, self.syn1.shape[0] - n_new)
        NamedTables(tables, m={}, v={}).take_over(taken, lambda k: k, rows.get, False)
