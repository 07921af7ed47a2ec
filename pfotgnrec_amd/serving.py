"""The serving surface of the model: everything a served ``TGN`` does between training steps - ``recommend`` (read-only),
``observe`` / ``ingest`` (state advance), the tables that grow (``reserve``, ``add_nodes``, ``add_edge_features``), the holdings
ledger, the retention window (``expire``) and erasure by node (``forget``).  A plain mixin that ``TGN`` inherits ahead of ``nn.Module``: the training step
calls nothing in here."""
import ctypes

import numpy as np
import torch

from . import _lib


def _check_log(batch_size, **columns):
    """The argument check ``observe`` and ``ingest`` open with, over ``name=(array, device dtype or None)`` columns of one log
    -> ``(on_dev, N, arrays)``.  The first column says whether the log is on the host or on the device; all columns have its
    length; ``batch_size`` is None or at least 1; on the device every column with a dtype is a 1-d tensor of it.  Host columns
    come back as numpy arrays, device columns as they are."""
    names, arrays = list(columns), [a for a, _ in columns.values()]
    on_dev = torch.is_tensor(arrays[0])
    N = int(arrays[0].shape[0]) if on_dev else len(arrays[0])
    if any(len(a) != N for a in arrays[1:]):
        raise ValueError("%s and %s must have the same length" % (", ".join(names[:-1]), names[-1]))
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError("batch_size must be at least 1")
    typed = [(a, dt) for a, dt in columns.values() if on_dev and dt is not None]
    if any((not torch.is_tensor(a)) or a.dtype != dt or a.dim() != 1 for a, dt in typed):
        raise ValueError("device inputs must be 1-d tensors " + " / ".join(str(dt)[6:] for _, dt in typed))
    return on_dev, N, arrays if on_dev else [np.asarray(a) for a in arrays]


class Serving:
    # ------------------------------------------------------------------ serving: read-only top-k
    def _embed_readonly(self, roots, root_ts, K):
        """Embeddings of (node, time) roots exactly as a forward would give them - pending messages applied lazily
        (tgn.py:251), L layers over the neighbours strictly before each root's time - with NOTHING written to the model: no
        persist, no message store, dropout 0 whatever ``train()`` says, the data-parallel sharding ignored.  The roots walk
        through the forward-only passes in chunks of ``eval_chunk_roots``.  The host-side step counter (position of the Philox
        streams: uniform sampling draws from it) and the "a GRU took part" flag are put back, so the next training step is the
        one it would have been."""
        K, root_ts = self._no_neighbours(int(K), root_ts)
        saved = (self._step, self._gru_applied_now)
        self._drop_prefetched()          # (a batch prepared ahead of time is simply prepared again by its own call)
        try:
            with torch.no_grad():
                emb, call = self._forward_chunks(roots, root_ts, K, 0.0, max(1, self._ws_caps[2]),
                                                 [(c0, None) for c0 in range(0, int(roots.shape[0]), max(1, int(self.eval_chunk_roots)))])
                if call is not None:
                    call.release()
        finally:
            self._step, self._gru_applied_now = saved
        return emb

    def _walk_readonly(self, roots, root_ts, K, visit):
        """The forward-only chunk walk of ``_embed_readonly`` for a query that reads the WORKSPACE of each pass and not its
        embeddings: ``visit(call, c0, c1)`` runs behind the pass over rows [c0, c1) and before that pass's workspace goes back to
        the pool (``_forward_chunks`` hands it back first).  ``K`` is past ``_no_neighbours`` already.  Nothing of the model is
        written; the step counter and the "a GRU took part" flag are put back."""
        R, cap, B = int(roots.shape[0]), max(1, int(self.eval_chunk_roots)), max(1, self._ws_caps[2])
        saved = (self._step, self._gru_applied_now)
        self._drop_prefetched()
        try:
            with torch.no_grad():
                for c0 in range(0, R, cap):
                    c1 = min(R, c0 + cap)
                    call = self._make_call(roots[c0:c1], root_ts[c0:c1], K, None, 0.0, None, B)
                    try:
                        self._native_forward(call)
                        visit(call, c0, c1)
                    finally:
                        call.release()
        finally:
            self._step, self._gru_applied_now = saved

    def explain(self, nodes, timestamps, m, hops=1, n_neighbors=None, return_raw=False):
        """WHY an embedding is what it is: the ``m`` past interaction partners the embedding of each (node, time) attends to most,
        most important first - "you are shown X because of your trades in A, B, C".  A query under ``recommend``'s contract: NO
        model state is written (memory, last_update, the pending-message tables, parameters, gradients and the step counter
        keep every bit; ``self.training`` is left as found), pending messages are applied lazily as every forward does, no
        gradient is recorded and dropout is off.

        nodes: [U] node ids (numpy / list, or an integer tensor) - users, or items to explain the item side of a pair;
        timestamps: a scalar or f64 [U] on host or device; m: 1 .. 256; hops: 1 or 2 (at most ``n_layers``); n_neighbors:
        default the model's.

        The numbers are the head-averaged softmax weights of the temporal attention layers (what ``nn.MultiheadAttention``
        returns beside its output, 0 on padding), read from the workspace of the forward-only pass by ``pfo_tgn_explain``
        (DESIGN §4s), in fp64: ``p[k] = (sum_h w[h, k]) / H``.  A sampled slot counts iff its neighbour is not the padding node.
        ``hops=1``: the weight of node v is the sum of the top layer's ``p[k]`` over the root's slots that name v - a user who
        traded one stock five times gets ONE entry with ``count`` 5.  ``hops=2`` (attention rollout): every two-hop path root ->
        slot j -> slot i of that neighbour's own row one layer down weighs ``p_L[j] * p_(L-1)[i]``, and the weight of v is the sum
        over the paths that end in v; the root's OWN row of the lower layer (its self path) is not part of the rollout, so a row
        sums to at most 1.  A ``hops=1`` row sums to 1 up to rounding, or to 0 when it is empty.

        Returns, on the device, ``(node i32[U, m], weight f64[U, m], n_valid i32[U], count i32[U, m], age f32[U, m],
        eidx i32[U, m])``: the distinct nodes by weight descending, then smaller age, then smaller id; ``n_valid`` = min(m,
        distinct nodes); ``count`` the slots (paths) merged into the entry; ``age`` the smallest dt among them - the root's time
        minus the edge's time, the value the time encoder saw, for a path that of its last edge - and ``eidx`` the edge id of
        that entry (among equal ages the lowest slot / path).  Slots beyond ``n_valid`` hold -1 / 0.0 / 0 / NaN / -1.  A row is
        empty when the node has no neighbour before its time, and every row is when ``n_neighbors`` <= 0.

        ``return_raw=True`` appends a dict of the per-slot tables the answer was made from, copied out of the workspace: ``nbr``
        i32[U, K], ``w`` f32[U, H, K], ``dt`` f32[U, K], ``eidx`` i32[U, K] of the top layer, and with ``hops=2`` ``nbr2``
        i32[U, K, K], ``w2`` f32[U, K, H, K], ``dt2``, ``eidx2`` of the neighbours' rows one layer down - the per-edge explanation
        the attention layer itself returns.

        Host inputs are checked (ValueError) before a device is asked for; node ids in a device tensor are not."""
        from . import explain as E
        query = E.validate(self.n_nodes, self.n_layers, self.n_neighbors, nodes, timestamps, m, hops, n_neighbors)
        _lib.require_gpu(self.device)
        return E.assemble(self, query, return_raw)

    def recommend(self, users, timestamps, k, items, exclude=None, item_ok=None, n_neighbors=None, return_embeddings=False,
                  mv=None, portfolios=None, day_idx=None, basket=False, *, portfolio_weights=None, held_groups=None, stock_groups=None,
                  seen_since=None, seen_width=None, seen_max_scan=0, only=None, groups=None, group_cap=None):
        """The ``k`` items of ``items`` this model would offer each user at its time, best first - a query: NO model state is
        written (memory, last_update, the pending-message tables, parameters and gradients keep every bit; ``self.training``
        is left as found), no gradient is recorded and dropout is off.

        users: [U] node ids (numpy / list, or an integer tensor); timestamps: a scalar or f64 [U]; items: [I] candidate item
        node ids, distinct and non-zero (shared by all users); exclude: None, a list of per-user lists of item NODE IDS (what
        the user already holds), or a packed pair (ids i32[U,W] padded with -1, lens i32[U]) - ids that are not in ``items``
        are ignored; item_ok: optional bool / u8 [I], 0 = never offer this candidate; n_neighbors: default the model's (20).

        Every (item, distinct timestamp) pair is embedded once (the grid of ``TGN._dedup_roots``), users and grid go through
        the forward-only chunk walk, and one launch of ``pfo_recommend_topk`` scores and selects.  Returns, on the device,
        (item_ids i32[U,k], scores f32[U,k], n_valid i32[U]): score descending, among equal scores the later entry of
        ``items`` first; slots beyond the admissible candidates hold id -1 and score -inf.  With
        ``return_embeddings`` also (user_emb [U,D], item_emb [n_t*I,D], user_block i32[U]): the block of n_t = number of
        distinct timestamps each user was scored against.

        With ``mv`` (an ``MVSampler``, or any object with ``returns``, ``upper_u``, ``gamma``, ``lambda_mv``, ``day_of``) the
        order is the mean-variance rank fusion the model is trained towards (main.py:243-289) over the whole candidate list:
        ``lambda_mv * rank(y_mv) + (1 - lambda_mv) * rank(score)``, one launch of ``pfo_recommend_mv_topk``.  portfolios: the
        stock indices each user holds, packed (port_idx i32[U,W], port_len i32[U]) on host or device, or a list of per-user
        lists (entries outside the return table are ignored; they weigh on y_mv, ``exclude`` still decides what is offered);
        day_idx: an int or one per user, None: ``mv.day_of(timestamps)`` (host timestamps only); a candidate's stock row is
        ``item - upper_u - 1``.  Up to 2048 candidates that is the one launch; beyond, up to 65536, the same list comes from
        ``pfo_recommend_mv_topk_wide``: ranks by sorting in a workspace of 36 bytes per user and candidate (256 MiB at the
        most, the users served in slabs), two launches a slab.  Returns (item_ids, scores, n_valid, fused f64[U,k]) - fused
        descending, -inf in empty slots - then the embeddings as above.

        ``basket=True`` (needs ``mv``): the list is taken one pick at a time - pick r is ranked with the stocks of picks
        0 .. r-1 counted as held behind the user's portfolio, so two near-identical stocks no longer both make the list; one
        launch of ``pfo_recommend_basket_topk`` in place of ``pfo_recommend_mv_topk``, equal to k calls with ``k=1`` and each
        pick appended to ``portfolios`` and ``exclude``.  The same return tuple; ``fused[u, r]`` is the pick's value in round r.
        The basket has no wide form: at most 2048 candidates.

        ``exclude="held"`` / ``portfolios="held"`` (either alone, or both): the rows of the holdings ledger
        (``track_holdings``) in place of the argument - one ``pfo_holdings_gather`` over the users already on the device, no
        lists packed or uploaded per query; ``portfolios="held"`` still needs ``mv``, whose ``upper_u`` must be the ledger's.

        ``mv`` may be a ``PriceLedger`` (prices.py): its return table grows by the day on the device.  ``day_idx`` is then the
        ordinal among the ledger's live days (0 = oldest); ``day_idx=None`` also takes DEVICE timestamps - one
        ``pfo_day_lookup``, no read-back - and a user whose day the ledger does not hold gets an empty answer there, where host
        timestamps raise ``KeyError``.

        ``only``: every user is offered the best of a list of its OWN - a watchlist, a tradable universe, what it holds - in
        place of all of ``items`` minus ``exclude``: a list of per-user lists of item NODE IDS (256 at the most), a packed pair
        (ids i32[U,W] padded with -1, lens i32[U]) on host or device, or ``"held"``: the user's row of the holdings ledger, from
        the one ``pfo_holdings_gather`` the query makes anyway.  Ids that are not in ``items`` are ignored, an id named twice
        counts once, an empty list gives an empty answer; ``item_ok`` still applies.  One launch of ``pfo_recommend_list_topk``,
        with ``mv`` of ``pfo_recommend_list_mv_topk``: both ranks run over the user's list alone, ``items`` may hold any number
        of candidates up to 65536 and no workspace is taken.  The portfolio is used as given: with ``portfolios="held"`` and
        ``only="held"`` a candidate is ranked against holdings it is itself among.  Not with ``exclude`` and not with
        ``basket=True`` (ValueError).  The scores are fp32 dot products in another summation order than the shared-list
        kernels': equal within the fp32 error bound, not to the bit.  The grid that is embedded is still every item of
        ``items`` - to embed less, pass the union of the lists as ``items``.  The return tuple is the same.

        ``groups`` with ``group_cap`` (both or neither): a concentration limit - at most ``group_cap`` (an int >= 1) items of a
        group in a user's list.  groups: one integer per entry of ``items`` - its sector, exchange, issuer, risk bucket; any
        non-negative int32, a negative id puts the item in no group and it is never capped - as a host array or list, or an
        integer device tensor (brought to int32 on the device once).  The order is the one served without the cap, walked with a
        candidate skipped when its group is full: ranks, scores and fused values are the uncapped ones, n_valid counts what was
        taken.  With ``basket=True`` a full group leaves the pool of the later rounds, like excluded items.  Still one launch
        (``pfo_recommend_topk_capped`` / ``pfo_recommend_mv_topk_capped`` / ``pfo_recommend_basket_topk_capped``) and the same
        return tuple.  Not with ``only`` (the list forms have no capped order) and, with ``mv``, not beyond 2048 candidates (the
        capped order has no wide form): ValueError.

        ``held_groups`` (with ``groups`` / ``group_cap``): the cap counts what a user already HOLDS - every holding named here
        uses up one slot of its group's quota, so a user who holds ``group_cap`` names of a sector is offered none of it, and one
        who holds one of two is offered one more.  Given as one list of group ids per user (one id per holding, the ids of
        ``groups``; a negative id: a holding in no group; an id named twice counts twice), as a packed pair (ids i32[U, W] padded
        with -1, lens i32[U]) on host or device, or by name: ``"held"`` - the rows of the holdings ledger, from the one gather the
        query makes anyway - or ``"portfolios"`` - the rows of ``portfolios=`` - both mapped on the device through
        ``stock_groups``, one integer per stock index (item node - upper_u - 1; an index outside it: no group).  At most 256 ids
        per user.  Still one launch (``pfo_recommend_topk_capped_held`` / ``pfo_recommend_mv_topk_capped_held`` /
        ``pfo_recommend_basket_topk_capped_held``); with no holding named, the lists are those of ``groups`` / ``group_cap`` alone.
        In the basket a group that the holdings alone fill takes part in no round.  (``held_groups``, ``stock_groups``, ``only``,
        ``groups`` and ``group_cap`` go by name.)

        ``exclude="seen"`` / ``only="seen"`` / ``portfolios="seen"`` (any of them, also beside ``"held"``): the rows come from the
        graph's own history - what the user's row of the temporal adjacency names STRICTLY before the user's query time (fp64 on
        the stored timestamps), distinct, newest first: "do not offer what this user has already traded", "rank the names this
        user has traded before", "the names traded are the portfolio".  No ledger and no lists packed per query: one
        ``pfo_history_gather`` over the finder's device CSR and the per-user timestamps already on the device serves whoever
        asks.  ``seen_since`` (a scalar or f64 [U] on host or device; None / NaN: no lower end) keeps the entries at or after that
        time only; ``seen_width`` (1 .. 256, default 256) is how many distinct names a user's row holds - the newest win;
        ``seen_max_scan`` > 0 looks at the newest that many entries of the window only.  ``portfolios="seen"`` needs ``mv``: a seen
        node is stock ``node - mv.upper_u - 1``, nodes outside the return table are ignored as always;
        ``held_groups="portfolios"`` maps these rows through ``stock_groups`` like any portfolio rows.  What is refused for
        explicit rows stays refused (``only`` with ``exclude``, ``basket=True`` or ``groups``); the three ``seen_*`` without any
        ``"seen"`` are refused too.  Entries removed by ``expire`` are no longer seen; interactions taken in by ``ingest`` /
        ``observe(append=True)`` are.

        ``portfolio_weights`` (with ``mv``; by name): every holding weighs on the mean-variance value by its size, not 1 /
        n_holding each - ``y = (mu / gamma - 0.5 * (1 / sum w) * sum_p w_p cov(i, p)) / var``, so a user with 95 % of the money in
        one stock is ranked against that stock.  Given as rows - one list of numbers per user matching ``portfolios`` entry for
        entry, or an f64 [U, W] array or tensor in the shape of packed ``portfolios`` - or by name beside ``portfolios="held"`` on a
        ledger made with ``quantities=True``: ``"shares"`` - the ledger's share counts - or ``"value"`` - share count x last close,
        which needs ``mv`` to be a ``PriceLedger`` on the ledger's ``upper_u``.  A holding whose weight is not finite and
        positive (a stock never quoted under ``"value"``) is left out like a stock outside the return table; all-ones rows give
        the unweighted lists bit for bit.  The named forms cost one ``pfo_holdings_gather_weights`` over the users already on the
        device: nothing is packed or read back.  ``"value"`` uses the ledger's NEWEST close whatever the query day is - the
        ledger keeps returns, not prices, per day.  One launch of ``pfo_recommend_mv_topk_weighted`` (beyond 2048 candidates
        ``pfo_recommend_mv_topk_wide_weighted``, with ``only`` ``pfo_recommend_list_mv_topk_weighted``).  Refused (ValueError):
        without ``mv``, with ``basket=True`` (the weight a pick joins the holdings with is undefined), with ``groups`` (the capped
        orders have no weighted form), with ``portfolios="seen"`` (the caller cannot align rows it never sees), explicit rows
        beside ``portfolios="held"``, a shape that is not the portfolios'.

        Host inputs are checked (ValueError); node ids in device tensors of ``users`` / ``exclude`` / ``only`` are not (it would
        cost a read-back).  ``items`` is read back once when it is a device tensor."""
        from . import recommend as R
        query = R.validate(self.n_nodes, self.n_neighbors, users, timestamps, k, items, exclude, item_ok, n_neighbors, mv,
                           portfolios, day_idx, self.holdings, basket, only, groups=groups, group_cap=group_cap,
                           held_groups=held_groups, stock_groups=stock_groups, seen_since=seen_since, seen_width=seen_width,
                           seen_max_scan=seen_max_scan, portfolio_weights=portfolio_weights)
        _lib.require_gpu(self.device)
        return R.assemble(self, query, return_embeddings)

    def history(self, users, timestamps, width, since=None, max_scan=0, items=None):
        """What each user interacted with before its time, read from the temporal adjacency the model's finder keeps on the
        device (``pfo_history_gather``) - a query: NO model state, ledger row or finder array is written.  Per user the distinct
        neighbours among the row entries with ``since <= t < timestamp`` (fp64, strict at the top), newest first, at most
        ``width`` (1 .. 256); ``max_scan`` > 0 looks at the newest ``max_scan`` entries of that window only.

        users: [U] node ids (host array or integer tensor); timestamps / since: a scalar or f64 [U] on host or device (since
        None / NaN: no lower end).  Returns, on the device, (nodes i32[U, width] padded with -1, lens i32[U], times f64[U, width]
        - the newest timestamp of each neighbour, NaN padding -, counts i32[U, width] - how many entries of the window name it),
        and with ``items`` (distinct candidate node ids) also positions i32[U, width]: the neighbour's place in ``items`` or -1.
        A non-finite timestamp gives an empty row.  Host ``users`` / ``items`` are checked like ``recommend``'s (ValueError for an
        id outside [0, n_nodes)); ids in a device tensor are not - one outside the finder's table gives an empty row.  Entries
        ``expire`` removed are gone."""
        from . import recommend as R
        users_h = R._int_vector(users, "users", self.n_nodes)
        U = int(users.shape[0]) if users_h is None else int(users_h.shape[0])
        since, width, max_scan = R.validate_seen(U, True, since, width, max_scan, names=("since", "width", "max_scan"))
        ts = timestamps if torch.is_tensor(timestamps) else np.asarray(timestamps)
        if ts.ndim != 0 and tuple(ts.shape) != (U,):
            raise ValueError("timestamps must be a scalar or hold one value per user (%d), got shape %s" % (U, tuple(ts.shape)))
        if not torch.is_tensor(ts) and ts.dtype.kind not in "fiu":
            raise ValueError("timestamps must be numbers")
        want = ("node", "len", "time", "count")
        items_d = None
        if items is not None:
            items_h = R._int_vector(items.detach().cpu().numpy() if torch.is_tensor(items) else items, "items", self.n_nodes)
            if not 1 <= items_h.shape[0] <= _lib.RECOMMEND_MAX_ITEMS:
                raise ValueError("items must hold between 1 and %d candidates (got %d)" % (_lib.RECOMMEND_MAX_ITEMS, items_h.shape[0]))
            if np.unique(items_h).shape[0] != items_h.shape[0]:
                raise ValueError("items holds duplicates")
            want += ("pos",)
        _lib.require_gpu(self.device)
        with torch.no_grad():
            if items is not None:
                items_d = R._to_dev(self.device, items_h, torch.int32)
            users_d = R._to_dev(self.device, users if users_h is None else users_h, torch.int32)
            ts_d = R._to_dev(self.device, ts, torch.float64).reshape(-1)
            ts_d = ts_d.expand(U) if ts.ndim == 0 else ts_d
            return R.seen_rows(self, users_d, ts_d, since, width, max_scan, want, items_d)

    # ------------------------------------------------------------------ serving: write-only state advance
    def _observe_workspace(self, B):
        """A workspace of ``pfo_tgn_observe`` from the pool (its entries carry the capacities (0, 0, 0): no forward takes them,
        and they go with the other undersized buffers when the step's workspace grows)."""
        need = _lib.byte_count("pfo_tgn_observe_workspace_bytes", ctypes.byref(self._cfg), B)
        for i, (caps, ws) in enumerate(self._ws_pool):
            if caps == (0, 0, 0) and ws.numel() >= need:
                return self._ws_pool.pop(i)[1]
        return torch.empty(need, dtype=torch.uint8, device=self.device)

    def observe(self, sources, destinations, edge_times, edge_idxs, batch_size=None, append=False):
        """Takes in interactions WITHOUT embedding anything - the write-only counterpart of ``recommend``: a chronological log
        is walked on the device in batches of ``batch_size`` and ``memory``, ``last_update`` and the pending-message tables
        end exactly where ``compute_temporal_embeddings[_p]`` would leave them batch by batch (tgn.py:295-317: the GRU on the
        batch's own positives that hold a message, the persist, the raw-message store) - no negatives, no sampling, no
        attention.  One native call (``pfo_tgn_observe``), no Python work per batch.  Nothing else is written: parameters,
        gradients, optimizer state, the step counter and the random streams stay as they are; no gradient is recorded
        whatever ``train()`` says.  Returns the number of interactions consumed.

        sources / destinations / edge_times / edge_idxs: numpy i64 / i64 / f64 / i64 like the entry points (range-checked:
        IndexError), or device tensors i32 / i32 / f64 / i32 (not checked: it would cost a read-back).  ``edge_idxs`` must
        address EXISTING rows of the edge-feature table: interactions whose features (or nodes) the model has never seen go
        through ``ingest``, which grows the tables and then calls this.
        ``batch_size``: interactions per batch, None = the whole input is one batch.  Batch boundaries are part of the
        semantics (messages are built from the memory as of their batch's persist): replay a log with the batch size it
        was - or would have been - trained with.  Chronological order is the caller's contract (``debug_checks`` asserts, like
        ``embed_device``, that no pending message is older than its node's last update).
        ``append``: the edges also go into the model's neighbour finder (``NeighborFinder.append``) behind the state update, so
        that a later ``recommend`` sees them; a ``GraphedTrainStep`` captured over the finder goes stale - as does one captured
        before ``reserve`` / ``add_nodes`` / ``add_edge_features`` moved or grew a table it holds the address of.  Off by default:
        a replay over a finder that already holds the log must not duplicate its edges.
        The data-parallel sharding is ignored (every rank observes the whole input: the state is replicated).
        Without memory there is no state: only the optional append happens."""
        on_dev, N, (sources, destinations, edge_times, edge_idxs) = _check_log(
            batch_size, sources=(sources, torch.int32), destinations=(destinations, torch.int32),
            edge_times=(edge_times, torch.float64), edge_idxs=(edge_idxs, torch.int32))
        if not on_dev:
            sources, destinations = self._check_nodes(sources, "sources"), self._check_nodes(destinations, "destinations")
            edge_idxs = self._check_edges(edge_idxs)
        if self.use_memory and N > 0:
            _lib.require_gpu(self.device)
            with torch.no_grad():
                self.join()                   # a side-stream optimizer step / a backward beside the host loop may still be running
                self._drop_prefetched()       # (its packed memory / message rows would be stale)
                if on_dev:
                    src, dst, ts, eidx = (a.contiguous() for a in (sources, destinations, edge_times, edge_idxs))
                else:
                    ts, src, dst, eidx = self._batch_to_dev([(edge_times, np.float64), (sources, np.int32), (destinations, np.int32),
                                                             (edge_idxs, np.int32)])
                if self.debug_checks:
                    m = self.memory
                    late = (m.has_msg > 0) & (m.last_update > m.msg_time)
                    assert not bool(late.any()), "Trying to update memory to time in the past"      # memory_updater.py:25,41
                B = N if batch_size is None else min(int(batch_size), N)
                ws = self._observe_workspace(B)
                st = self._state_struct(adjacency=False)
                try:
                    _lib.call("pfo_tgn_observe", ctypes.byref(self._cfg), ctypes.byref(st), src.data_ptr(), dst.data_ptr(),
                              ts.data_ptr(), eidx.data_ptr(), N, B, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
                finally:
                    self._ws_pool.append(((0, 0, 0), ws))
                self.memory._any_msg = True
                self.memory._state_version += 1
        if append and N > 0:
            host = (lambda a: a.cpu().numpy()) if on_dev else np.asarray
            self.neighbor_finder.append(host(sources), host(destinations), host(edge_idxs), host(edge_times))
        return N

    # ------------------------------------------------------------------ serving: tables that grow
    @property
    def edge_feature_stats(self):
        """``(mean f32[Ef], std f32[Ef])`` on the host: the column statistics the constructor normalised the edge-feature
        table with - the mean of the table, the standard deviation of the centred table, both fp32 as numpy computed them.
        FROZEN: rows added later (``add_edge_features``) are scaled with these and never with recomputed ones - the weights
        were trained against this scaling.  They are NOT part of ``state_dict()`` (existing checkpoints keep loading): a model
        restored next to a table that has grown since takes them from ``set_edge_feature_stats``."""
        return self._edge_stats

    def _set_stats(self, mean, std):
        mean = np.ascontiguousarray(np.asarray(mean), dtype=np.float32).reshape(-1)
        std = np.ascontiguousarray(np.asarray(std), dtype=np.float32).reshape(-1)
        self._edge_stats = (mean, std)
        self._edge_stats_dev = torch.from_numpy(np.stack([mean, std])).to(self.device).contiguous()     # [2, Ef]: mean | std

    def set_edge_feature_stats(self, mean, std):
        """Replaces the frozen statistics (``edge_feature_stats``), e.g. with those saved beside a checkpoint.  The table is
        NOT re-normalised: only rows added from now on are scaled with the new vectors."""
        mean, std = np.asarray(mean), np.asarray(std)
        if mean.shape != (self.n_edge_features,) or std.shape != (self.n_edge_features,):
            raise ValueError("mean and std must have shape (%d,)" % self.n_edge_features)
        self._set_stats(mean, std)

    node_capacity = property(lambda self: self._nodes.capacity)
    edge_capacity = property(lambda self: self._edges.capacity)

    def _quiesce(self):
        # a side-stream optimizer step / a backward beside the host loop may still read the tables that are about to move
        if self._flat.is_cuda:
            self.join()
            self._drop_prefetched()

    def reserve(self, n_nodes=None, n_edges=None):
        """Capacity for ``n_nodes`` rows of the node tables (``node_raw_features``, ``memory.memory``, ``memory.last_update``,
        the pending-message table, its times and flags) and ``n_edges`` rows of the edge-feature table - rows, the padding
        row 0 included.  Live rows are copied across bit for bit, rows behind them are zero; the attributes stay what they
        were - contiguous leading-row views of the storage, same dtypes and shapes - but their addresses change when storage
        is reallocated.  Capacity never shrinks (asking for what is there, or less, does nothing); asking for less than the
        live rows raises ``ValueError``.  Without ``reserve`` the tables grow geometrically on demand.  Call it between steps
        (see ``add_nodes``); a ``GraphedTrainStep`` captured before goes stale."""
        for what, want, store in (("n_nodes", n_nodes, self._nodes), ("n_edges", n_edges, self._edges)):
            if want is not None and int(want) < store.rows:
                raise ValueError("reserve(%s=%d) is below the %d live rows" % (what, int(want), store.rows))
        # (the memory tables and the ledger follow the node capacity)
        for want, store, followers in ((n_edges, self._edges, ()), (n_nodes, self._nodes, (self.memory, self.holdings))):
            if want is not None and int(want) > store.capacity:
                self._quiesce()
                store.reserve(want)
                for tables in followers:
                    if tables is not None:
                        tables.resize(store.rows, want)
                self._tables_changed(rows=False)
        return self

    def add_edge_features(self, raw):
        """Appends ``raw`` f32[m, Ef] RAW edge-feature rows - a host array (checked: width, finite values; staged through the
        batch ring) or an fp32 device tensor (shape checked only) - behind the live rows, normalised with the frozen
        ``edge_feature_stats`` by ONE launch of ``pfo_edge_rows_append`` (numpy's two fp32 operations, bit for bit).  Returns
        the new rows' edge indices, i64[m]: the old row count onwards.  Nothing else changes; live rows keep every bit (they
        move only when the capacity is exceeded: ``reserve``)."""
        Ef = self.n_edge_features
        if torch.is_tensor(raw):
            if raw.dim() != 2 or raw.shape[1] != Ef or raw.dtype != torch.float32:
                raise ValueError("device edge features must be an fp32 tensor [m, %d]" % Ef)
            dev_rows = raw
        else:
            raw = np.asarray(raw)
            if raw.ndim != 2 or raw.shape[1] != Ef:
                raise ValueError("edge features must have shape [m, %d], got %s" % (Ef, raw.shape))
            raw = raw.astype(np.float32, copy=False)
            if not np.isfinite(raw).all():
                raise ValueError("edge features must be finite")
            dev_rows = None
        m, n0 = int(raw.shape[0]), int(self.edge_raw_features.shape[0])
        if n0 + m >= 2 ** 31:
            raise ValueError("edge indices must fit in int32")
        if m == 0:
            return np.zeros(0, np.int64)
        _lib.require_gpu(self.device)
        if dev_rows is None:
            dev_rows = self._batch_to_dev([(raw, np.float32)])[0]
        dev_rows = dev_rows.contiguous()
        if n0 + m > self.edge_capacity:           # (every tick comes through here: no call when the rows fit)
            self.reserve(n_edges=self._edges.capacity_for(n0 + m))
        st = self._edge_stats_dev
        _lib.call("pfo_edge_rows_append", dev_rows.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), m, Ef, self.edge_raw_features.data_ptr(),
                  n0, self.edge_capacity, _lib.stream_ptr())
        self._edges.set_rows(n0 + m)
        self._point_edges()
        return np.arange(n0, n0 + m, dtype=np.int64)

    def add_nodes(self, n, node_features=None):
        """``n`` new nodes behind the last one; returns the first new node id (= the old ``n_nodes``).  Their rows of
        ``node_raw_features`` are ``node_features`` f32[n, D] or zeros (the reference's node features are all zeros,
        main.py:87); their memory, last update and pending-message state are the initial ones (zero, none pending).
        Parameters, their ``.grad`` views, the flat buffers, the optimizer state, the step counter and the parameter cache
        (its size does not depend on the node count) are untouched.  Invalidated: the workspace pool (workspaces are carved
        per node count), the padded device adjacency, a batch prepared ahead of time, the ``debug_*`` views of the last
        forward, and any ``GraphedTrainStep`` captured before.

        Call it BETWEEN steps: a forward whose backward is still pending keeps the workspace and config it ran with, and must
        have its backward run first."""
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        D = self.n_node_features
        rows = None
        if node_features is not None:
            rows = node_features if torch.is_tensor(node_features) else torch.from_numpy(
                np.ascontiguousarray(np.asarray(node_features), dtype=np.float32))
            if rows.dim() != 2 or tuple(rows.shape) != (n, D):
                raise ValueError("node_features must have shape [%d, %d], got %s" % (n, D, tuple(rows.shape)))
        first = self.n_nodes
        if n == 0:
            return first
        if first + n >= 2 ** 31:
            raise ValueError("node ids must fit in int32")
        self._quiesce()
        self.reserve(n_nodes=self._nodes.capacity_for(first + n))
        self._nodes.set_rows(first + n)
        for tables in (self.memory, self.holdings):               # (rows behind the live ones hold the initial values already;
            if tables is not None:                                #  the memory bumps its _state_version)
                tables.resize(first + n)
        self._tables_changed(node_count=True)
        if rows is not None:                                      # (the new rows were zero)
            self.node_raw_features[first:].copy_(rows.to(dtype=torch.float32))
        return first

    def ingest(self, sources, destinations, edge_times, edge_features, batch_size=None, node_features=None, portfolios=None):
        """The serving tick: takes in interactions the model has NEVER seen - their feature rows are not in the edge-feature
        table, their nodes may not exist yet - so that the next ``recommend`` accounts for them.  A thin chain of
        ``add_nodes`` (when the input names new nodes), ``add_edge_features`` and ``observe(..., append=True)``: the state
        semantics are ``observe``'s by shared code (batch boundaries included: ``batch_size``), every rank of a data-parallel
        group ingests the whole input, and nothing else is written.  Per tick: one launch for the feature rows, ONE
        ``pfo_tgn_observe`` call (4 launches per batch) and the CSR append; no Python work per batch.  Without memory only the
        tables and the finder grow.  Returns ``(n_consumed, edge_idxs i64[N])`` - the indices the new rows got.

        sources / destinations / edge_times: numpy i64 / i64 / f64 like ``observe``; edge_features: RAW rows f32[N, Ef]
        (normalised here with the frozen ``edge_feature_stats``).  Node ids >= ``n_nodes`` are allowed only as exactly the
        next consecutive ids; those nodes are added first, with ``node_features`` f32[n_new, D] as their rows in ascending id
        order, zeros otherwise.  Host inputs are validated BEFORE anything is written (``ValueError``: lengths, feature width,
        non-finite features, decreasing ``edge_times``, node ids < 1, ids that skip ahead, ``batch_size`` < 1): a rejected call
        leaves the model bit for bit as it was.  Device tensors (i32 / i32 / f64 and f32[N, Ef]) are checked for shape and
        dtype only and must name existing nodes (``add_nodes`` first).

        ``portfolios``: what each record says its user holds at that moment, in a form ``update_holdings`` takes (host forms
        with host inputs, the device pair with device inputs); needs a ledger (``track_holdings``).  Its checks join the ones
        above - a rejected call leaves the ledger too - and the ledger is written ONCE per call behind ``add_nodes`` (last
        record per user over the whole input: batch boundaries do not matter to it).  None: the ledger is not touched.

        ``portfolios="buys"``: the interactions themselves are the feed - every ingested interaction is a buy of stock
        ``destination - upper_u - 1`` by its source (quantity 1.0 on a ledger with quantities), applied to the ledger by
        ``pfo_holdings_apply`` once per call, where the snapshot is written otherwise: the ledger ends where ``ingest`` followed
        by ``trade_holdings`` of the same interactions leaves it.  A destination that is not an item node gives a negative
        stock and is skipped by the kernel's rule."""
        if portfolios is not None and self.holdings is None:
            raise ValueError("portfolios need a holdings ledger: call track_holdings(width, upper_u) first")
        buys = isinstance(portfolios, str) and portfolios == "buys"
        if portfolios is not None and not buys and self.holdings.quantities:
            raise ValueError("a ledger with quantities is written by trades only: portfolios=\"buys\" or trade_holdings")
        on_dev, N, (sources, destinations, edge_times, edge_features) = _check_log(
            batch_size, sources=(sources, torch.int32), destinations=(destinations, torch.int32),
            edge_times=(edge_times, torch.float64), edge_features=(edge_features, None))
        Ef, n_new = self.n_edge_features, 0
        if on_dev:
            if not torch.is_tensor(edge_features) or edge_features.dim() != 2 or edge_features.shape[1] != Ef or edge_features.dtype != torch.float32:
                raise ValueError("device edge features must be an fp32 tensor [N, %d]" % Ef)
            if node_features is not None:
                raise ValueError("device inputs must name existing nodes: add_nodes first")
        else:
            edge_times = np.asarray(edge_times, np.float64)
            if sources.ndim != 1 or destinations.ndim != 1 or edge_times.ndim != 1:
                raise ValueError("sources, destinations and edge_times must be 1-d")
            if edge_features.ndim != 2 or edge_features.shape[1] != Ef:
                raise ValueError("edge features must have shape [N, %d], got %s" % (Ef, edge_features.shape))
            if not np.isfinite(edge_features).all():
                raise ValueError("edge features must be finite")
            if N and (not np.isfinite(edge_times).all() or (np.diff(edge_times) < 0).any()):
                raise ValueError("edge_times must be finite and chronological (non-decreasing)")
            ids = np.concatenate([sources, destinations]).astype(np.int64)
            if N and int(ids.min()) < 1:
                raise ValueError("node ids must be >= 1 (node 0 is the padding node)")
            fresh = np.unique(ids[ids >= self.n_nodes])
            n_new = int(fresh.shape[0])
            if n_new and not np.array_equal(fresh, np.arange(self.n_nodes, self.n_nodes + n_new)):
                raise ValueError("new node ids must be exactly the next consecutive ids %d.. : got %s"
                                 % (self.n_nodes, fresh[:8].tolist()))
            if node_features is not None and tuple(np.shape(node_features)) != (n_new, self.n_node_features):
                raise ValueError("node_features must have shape [%d, %d]: one row per new node" % (n_new, self.n_node_features))
        held = None
        if portfolios is not None and not buys:   # (the new nodes are rows of the ledger by the time it is written)
            from . import holdings as H
            held = H.validate(self.holdings.width, self.n_nodes + n_new, sources, portfolios, edge_times)
        if N == 0:
            return 0, np.zeros(0, np.int64)
        _lib.require_gpu(self.device)             # (nothing below has a host path: refuse before the first table grows)
        if n_new:
            self.add_nodes(n_new, node_features)
        if held is not None:
            self._write_holdings(held)
        if buys:
            self._buy_holdings(sources, destinations, edge_times)
        new_idxs = self.add_edge_features(edge_features)
        eidx = torch.arange(int(new_idxs[0]), int(new_idxs[0]) + N, dtype=torch.int32, device=self.device) if on_dev else new_idxs
        return self.observe(sources, destinations, edge_times, eidx, batch_size, append=True), new_idxs

    # ------------------------------------------------------------------ serving: the holdings ledger
    def track_holdings(self, width, upper_u, quantities=False):
        """Creates the holdings ledger (``self.holdings``, None before): per node row the portfolio its user's newest
        interaction record carried - ``idx`` i32[n_nodes, width] STOCK indices padded with -1 (the packed form of
        ``pack_portfolios``; the item node of stock ``s`` is ``s + upper_u + 1``), ``len`` i32[n_nodes], ``time`` f64[n_nodes]
        (-1 / 0 / -inf until written) - in capacity storage that follows ``node_capacity`` (``reserve`` / ``add_nodes`` keep
        live rows bit for bit) and the model's device.  ``update_holdings`` and ``ingest(portfolios=)`` write it from snapshots,
        ``trade_holdings``, ``ingest(portfolios="buys")`` and ``backtest(advance_holdings=True)`` from trades,
        ``recommend(exclude="held", portfolios="held")`` and ``holdings.rows(users)`` read it; the training step, ``observe``
        and ``expire`` do not touch it, and it is not part of ``state_dict()``: persist ``holdings.idx / len / time`` and load
        them with ``update_holdings``.  Once: a second call with other arguments raises ``ValueError``.  Returns the ledger.

        ``quantities=True``: the ledger also keeps ``qty`` f64[n_nodes, width], the share count of every slot (0.0 at and behind
        ``len``), in the same capacity storage.  Such a ledger is written by trades only (``trade_holdings``,
        ``ingest(portfolios="buys")``): the snapshot writers raise ``ValueError`` on it, a snapshot carries no share counts."""
        from . import holdings as H
        quantities = bool(quantities)
        try:
            width, upper_u = int(width), int(upper_u)
        except (TypeError, ValueError):
            raise ValueError("width and upper_u must be integers") from None
        if not 1 <= width <= H.MAX_WIDTH:
            raise ValueError("width must lie in [1, %d] (got %d)" % (H.MAX_WIDTH, width))
        if not 0 <= upper_u < 2 ** 31 - 1:
            raise ValueError("upper_u must be a non-negative int32 (got %d)" % upper_u)
        if self.holdings is not None:
            if (self.holdings.width, self.holdings.upper_u, self.holdings.quantities) != (width, upper_u, quantities):
                raise ValueError("the model already tracks holdings with width %d, upper_u %d, %s quantities"
                                 % (self.holdings.width, self.holdings.upper_u, "with" if self.holdings.quantities else "without"))
            return self.holdings
        self.holdings = H.Holdings(self.n_nodes, self.node_capacity, width, upper_u, self.device, quantities)
        return self.holdings

    def update_holdings(self, sources, portfolios, edge_times):
        """The snapshot writer of the ledger (``trade_holdings`` is the other writer, and the only one of a ledger with
        quantities): for every event in input order, ``holdings[sources[e]] = (portfolios[e], edge_times[e])``
        - per user the LAST event of the call wins, an empty portfolio overwrites, entries are stored verbatim, nothing is
        compared with the stored time (chronological input is the caller's contract, as for ``observe``); node 0 is skipped.
        One native call (``pfo_holdings_store``: a memset and two launches).  Seeds a served model from the training log and
        loads a saved ledger (``sources = arange(n_nodes)``, ``portfolios = (idx, len)``, ``edge_times = time``).

        ``portfolios``: a packed pair (idx [N, Wp], len [N]) as numpy, one list of integer stock indices per event, or the pair
        as i32 device tensors next to i32 / f64 device ``sources`` / ``edge_times``.  Host inputs are validated before anything
        is written (``ValueError``: lengths, integer dtypes, values beyond int32, len outside [0, Wp], a row longer than the
        ledger's width, node ids outside [0, n_nodes)) and staged in one copy; device inputs are checked for shape and dtype
        only - the kernel skips ids outside [1, n_nodes) and clamps lengths to the row.  Returns the number of events."""
        if self.holdings is None:
            raise ValueError("no holdings ledger: call track_holdings(width, upper_u) first")
        if self.holdings.quantities:
            raise ValueError("a ledger with quantities is written by trades only: trade_holdings")
        from . import holdings as H
        w = H.validate(self.holdings.width, self.n_nodes, sources, portfolios, edge_times)
        if w.N:
            _lib.require_gpu(self.device)
            self._write_holdings(w)
        return w.N

    def _write_holdings(self, w):
        with torch.no_grad():
            if w.on_dev:
                src, idx, length, ts = w.src, w.idx, w.len, w.ts
            else:
                ts, src, idx, length = self._batch_to_dev([(w.ts, np.float64), (w.src, np.int32), (w.idx, np.int32), (w.len, np.int32)])
            self.holdings.store(src, idx, length, ts)

    def trade_holdings(self, sources, stocks, sides, edge_times, quantities=None):
        """The ledger's second writer: a feed of trades applied to the rows in event order on the device - one native call
        (``pfo_holdings_apply``), no row read back.  Event e: user ``sources[e]``, STOCK index ``stocks[e]``,
        ``sides[e]`` +1 (buy) or -1 (sell), time ``edge_times[e]``, and on a ledger with quantities ``quantities[e]`` shares (None:
        1.0 each).  A buy of a stock the row holds adds to its share count (nothing without quantities), of another one appends it
        behind the row's entries - a full row stays as it is and counts as an overflow.  A sell takes from the count; when
        nothing is left, and always without quantities, the position is closed and the entries behind it move one slot to the
        front (a row lists positions oldest first); a sell of a stock the row does not hold counts as unmatched.  Every event
        sets the row's time; nothing is compared with the stored time.  ``holdings_counters()`` reads the two counts.

        Host inputs are validated before anything is written (``ValueError``: lengths, integer dtypes, values beyond int32, node
        ids outside [0, n_nodes), sides outside {-1, +1}, quantities that are not finite and positive) - a rejected call leaves
        the ledger bit for bit - and staged in one copy.  Device inputs (i32 / i32 / i32 / f64 [/ f64]) are checked for shape and
        dtype only: the kernel skips an event with a user outside [1, n_nodes), a negative stock, another side or such a
        quantity, whole.  ``quantities=`` on a ledger without them raises ``ValueError``.  Returns the number of events.

        A saved ledger reloads through here: one buy per stored slot in slot order at the row's time (with its share count on
        a ledger with quantities) reproduces every row with ``len > 0`` bit for bit; a row with ``len == 0`` keeps time -inf."""
        if self.holdings is None:
            raise ValueError("no holdings ledger: call track_holdings(width, upper_u) first")
        from . import holdings as H
        t = H.validate_trades(self.n_nodes, self.holdings.quantities, sources, stocks, sides, edge_times, quantities)
        if t.N:
            _lib.require_gpu(self.device)
            with torch.no_grad():
                if t.on_dev:
                    cols = [c if c is None else c.contiguous() for c in (t.src, t.stock, t.side, t.ts, t.qty)]
                else:
                    host = [(t.ts, np.float64)] + ([(t.qty, np.float64)] if t.qty is not None else []) + [
                        (t.src, np.int32), (t.stock, np.int32), (t.side, np.int32)]
                    dev = self._batch_to_dev(host)
                    cols = [dev[-3], dev[-2], dev[-1], dev[0], dev[1] if t.qty is not None else None]
                self.holdings.apply(*cols)
        return t.N

    def holdings_counters(self):
        """``(overflow, unmatched)`` since the ledger was made - buys that found their row full, sells of a stock the row did not
        hold - read back from the device (the one synchronisation; no write makes it)."""
        if self.holdings is None:
            raise ValueError("no holdings ledger: call track_holdings(width, upper_u) first")
        return tuple(int(v) for v in self.holdings.counters.cpu().tolist())

    def _buy_holdings(self, sources, destinations, edge_times):
        """Interactions (host arrays or device tensors, validated by the caller) as buys of stock ``destination - upper_u - 1``."""
        h = self.holdings
        with torch.no_grad():
            if torch.is_tensor(sources):
                src, dst, ts = (a.contiguous() for a in (sources, destinations, edge_times))
            else:
                ts, src, dst = self._batch_to_dev([(np.asarray(edge_times), np.float64), (np.asarray(sources), np.int32),
                                                   (np.asarray(destinations), np.int32)])
            h.apply(src, dst - (h.upper_u + 1), torch.ones_like(src), ts)

    # ------------------------------------------------------------------ serving: the retention window
    def expire(self, cutoff, compact_edges=True, finders=None):
        """"Keep the last N days": every adjacency entry with ``ts < cutoff`` (strict, fp64) leaves the neighbour finder
        (``NeighborFinder.expire``) and, with ``compact_edges``, the rows of the edge-feature table that only expired entries
        named are released.  Returns ``(n_entries_dropped, remap)``: the entries dropped over all finders taking part, and the
        DEVICE tensor ``remap`` i32[old row count] - old edge index -> new one, ``remap[0] == 0``, -1 for a released row - or
        ``None`` when ``compact_edges=False`` or no row was released (edge indices then mean what they meant).

        The table is shared between finders (a train finder and a full finder over one table): ``finders`` names the OTHER
        ``NeighborFinder``s over this model's table; the model's own finder always takes part.  All are expired with the same
        cutoff and remapped with the same map.  A row ``r >= 1`` is released iff some expired entry of a finder taking part
        names it and no surviving entry of any of them does; rows nobody names stay, row 0 always stays.  A finder over this
        table that is NOT passed keeps its old edge indices and is wrong afterwards.  Surviving rows keep their order and are
        renumbered densely; they move down inside the unchanged storage through a temporary (``pfo_edge_rows_compact``), the
        rows behind the new live count are zero again, capacity never shrinks, and the next ``add_edge_features`` / ``ingest``
        continues from the new row count.

        Order: ``_quiesce()``, the finders, then the table.  Node memory, ``last_update``, the pending messages (they hold the
        feature VALUES, not edge indices), parameters, gradients, optimizer state, the step counter and the random streams are
        not touched.  Invalidated after a compaction: the padded device adjacency, the ``debug_*`` views of the last forward,
        a batch prepared ahead of time and any ``GraphedTrainStep`` captured before (an expiry alone already stales the
        latter through the finder's version).  Two read-backs (the surviving entry total per finder, the new row count): a
        maintenance call, not a step.

        Call it BETWEEN steps, like ``add_nodes``: a forward whose backward is still pending must have that backward run
        first.  On a data-parallel group EVERY rank calls it with the same cutoff: state is replicated, there is no
        collective.  ``cutoff`` must be finite (``ValueError`` before anything is written); without a device it raises like
        every compute method."""
        cutoff = float(cutoff)
        if not np.isfinite(cutoff):
            raise ValueError("the cutoff must be finite, got %r" % cutoff)
        _lib.require_gpu(self.device)
        taking_part = self._finders_over_table(finders, compact_edges)
        self._quiesce()
        flags = self._edge_row_flags() if compact_edges else None
        dropped = sum(nf.expire(cutoff, self.device, _row_flags=flags) for nf in taking_part)
        if not compact_edges or dropped == 0:                        # (nothing expired: nothing can be released)
            return dropped, None
        return dropped, self._release_edge_rows(flags, taking_part)

    def _finders_over_table(self, finders, compact_edges):
        """The finders a removal runs over: the model's own, then ``finders`` (each once).  Before a compaction every one of
        them must name rows of this table only (``ValueError``)."""
        taking_part = [self.neighbor_finder]
        for nf in (finders or ()):
            if not any(nf is f for f in taking_part):
                taking_part.append(nf)
        n_rows = int(self.edge_raw_features.shape[0])
        if compact_edges:
            for nf in taking_part:
                if nf.max_edge_idx() >= n_rows:
                    raise ValueError("a neighbour finder references edge index %d but edge features have %d rows"
                                     % (nf.max_edge_idx(), n_rows))
        return taking_part

    def _edge_row_flags(self):
        return torch.zeros(int(self.edge_raw_features.shape[0]), dtype=torch.int32, device=self.device)

    def _release_edge_rows(self, flags, taking_part):
        """The table side of ``expire`` and ``forget``, behind the finders: ``flags`` (``pfo_edge_rows_mark[_nodes]`` over every
        finder taking part) decide which rows are released, the kept ones move down, the finders' edge indices follow.
        Returns the device ``remap``, or None when no row was released (nothing was written then)."""
        n_rows, Ef = int(self.edge_raw_features.shape[0]), self.n_edge_features
        nbytes = _lib.byte_count("pfo_edge_rows_plan_scratch_bytes", n_rows)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        remap = torch.empty(n_rows, dtype=torch.int32, device=self.device)
        n_keep_dev = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.call("pfo_edge_rows_plan", flags.data_ptr(), n_rows, remap.data_ptr(), n_keep_dev.data_ptr(), scratch.data_ptr(),
                  nbytes, _lib.stream_ptr())
        n_keep = int(n_keep_dev.item())
        if n_keep == n_rows:
            return None
        tmp = torch.empty((n_keep, Ef), dtype=torch.float32, device=self.device)
        _lib.call("pfo_edge_rows_compact", self.edge_raw_features.data_ptr(), n_rows, n_keep, Ef, remap.data_ptr(), tmp.data_ptr(),
                  _lib.stream_ptr())
        for nf in taking_part:
            nf.remap_edge_idxs(remap, self.device)
        self._edges.trim(n_keep)                  # (the kernel zeroed the rows behind the new live count)
        self._tables_changed()
        return remap

    # ------------------------------------------------------------------ serving: erasure by node
    def _forget_ids(self, nodes):
        """``forget``'s argument check -> the ids as a numpy int32 array (host input, fully checked: ``ValueError``) or as the
        device tensor they came in (shape and dtype only: reading the ids would cost a read-back)."""
        if torch.is_tensor(nodes):
            if nodes.dim() != 1 or nodes.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64):
                raise ValueError("nodes must be a 1-d integer tensor of node ids")
            return nodes
        ids = np.asarray(nodes)
        if ids.ndim > 1:
            raise ValueError("nodes must be a flat list of node ids, got shape %s" % (ids.shape,))
        ids = ids.reshape(-1)
        if ids.size == 0:
            return np.zeros(0, np.int32)
        if ids.dtype.kind not in "iu":
            raise ValueError("node ids must be integers, got %s" % ids.dtype)
        if int(ids.min()) == 0:
            raise ValueError("node 0 is the padding node and cannot be forgotten")
        if int(ids.min()) < 1 or int(ids.max()) >= self.n_nodes:
            raise ValueError("node ids must lie in [1, %d): found %d .. %d" % (self.n_nodes, int(ids.min()), int(ids.max())))
        return ids.astype(np.int32)

    def forget(self, nodes, compact_edges=True, finders=None):
        """Erasure by node - ``expire``'s sibling, by node instead of by time: an account is closed and its history has to go,
        a stock is delisted, an id was ingested by mistake.  Every adjacency entry that touches a node of ``nodes`` leaves the
        neighbour finder (``NeighborFinder.forget``: the node's own row and the entries of other rows that name it), with
        ``compact_edges`` the rows of the edge-feature table that only those entries named are released, and the node's own
        rows return to what ``add_nodes`` gives a new node: memory, ``last_update``, the pending message, its time and flag
        and the node-feature row to zero, the holdings ledger's row (when there is a ledger) to (-1.., 0, -inf; its share
        counts to 0.0 by a fill) - ONE launch of
        ``pfo_node_rows_reset``, also for a node that had no adjacency entry.  Returns ``(n_entries_dropped, remap)`` exactly
        as ``expire`` does: the entries dropped over all finders taking part, and the device tensor ``remap`` i32[old row
        count] (old edge index -> new one, -1 for a released row), or ``None`` when ``compact_edges=False`` or no row was
        released.

        ``nodes``: a host list / array of node ids, or an integer device tensor.  Host ids are checked before anything is
        written (``ValueError``): they must be integers, node 0 (the padding node) is refused, ids outside ``[1, n_nodes)``
        are refused; duplicates are fine.  Device ids are not read back - the kernels skip ids outside ``[1, n_nodes)``.  An
        empty list returns ``(0, None)`` with nothing written.  ``finders`` names the OTHER finders over this model's table, as
        for ``expire``: all are swept with the same ids and remapped with the same map, and a finder over this table that is
        not passed is wrong afterwards.

        Order: ``_quiesce()``, the finders, the node rows, then the table.  Left untouched, bit for bit: parameters and
        gradients, optimizer state, the step counter, the random streams and every row of a node that is not forgotten.
        Invalidated: what ``expire`` invalidates (the finders' versions stale a captured ``GraphedTrainStep``; after a
        compaction the padded device adjacency, the ``debug_*`` views of the last forward and a batch prepared ahead of
        time); in addition the memory's ``_state_version`` is bumped (packed copies of memory rows are stale).  The host-side
        "some message is pending" knowledge is never lowered.  A forgotten id stays valid and reusable: ``ingest`` /
        ``observe`` may name it again, and it then starts like a new node.  ``history``, ``exclude="seen"`` and
        ``only="seen"`` read the finder and follow at once.

        THE LIMIT: what OTHER nodes hold stays.  Their memory and pending messages were computed from past interactions with
        the forgotten node; they hold derived values, not ids, and they are not recomputed (that takes a replay of the log
        without the node).  Other users' holdings rows that name a forgotten stock stay too: ``item_ok`` at query time or
        ``update_holdings`` deal with those.

        Call it BETWEEN steps, like ``add_nodes`` and ``expire``.  On a data-parallel group EVERY rank calls it with the
        same ids: state is replicated, there is no collective.  Two read-backs at the most per call (the surviving entry total
        per finder, the new row count); without a device it raises like every compute method."""
        ids = self._forget_ids(nodes)
        if int(ids.shape[0]) == 0:
            return 0, None
        _lib.require_gpu(self.device)
        n, m, h = self.n_nodes, self.memory, self.holdings
        floats = [self.node_raw_features] + ([] if m is None else [m.memory, m.last_update, m.msg_table, m.msg_time])
        if any(t.dtype != torch.float32 for t in floats):
            raise _lib.PfoError("the node tables must be fp32 to be reset on the device")
        taking_part = self._finders_over_table(finders, compact_edges)
        self._quiesce()
        with torch.no_grad():
            ids = torch.as_tensor(ids).to(device=self.device, dtype=torch.int32).contiguous()
            flags = self._edge_row_flags() if compact_edges else None
            dropped = sum(nf.forget(ids, self.device, _row_flags=flags) for nf in taking_part)
            gone = torch.empty(n, dtype=torch.uint8, device=self.device)
            _lib.call("pfo_nodes_flag", ids.data_ptr(), int(ids.shape[0]), n, gone.data_ptr(), _lib.stream_ptr())
            mem =[None, 0, None, None, 0, None, None] if m is None else [
                m.memory.data_ptr(), int(m.memory.shape[1]), m.last_update.data_ptr(), m.msg_table.data_ptr(), int(m.msg_table.shape[1]),
                m.msg_time.data_ptr(), m.has_msg.data_ptr()]
            held = [None, 0, None, None] if h is None else [h.idx.data_ptr(), h.width, h.len.data_ptr(), h.time.data_ptr()]
            _lib.call("pfo_node_rows_reset", gone.data_ptr(), n, *mem, self.node_raw_features.data_ptr(), self.n_node_features,
                      *held, _lib.stream_ptr())
            if h is not None and h.quantities:                       # (not the hot path: a fill by the same flags)
                h.qty.masked_fill_(gone.bool().unsqueeze(1), 0.0)
            if m is not None:
                m._state_version += 1
        if not compact_edges or dropped == 0:                        # (no entry went: no row can be released)
            return dropped, None
        return dropped, self._release_edge_rows(flags, taking_part)
