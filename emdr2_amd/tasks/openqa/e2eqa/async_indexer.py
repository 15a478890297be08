"""Continuous evidence re-indexing during training (BASELINE configs[5]).

Reference: tasks/openqa/e2eqa/async_indexer.py:84-144 runs `IndexBuilder` on a second group of GPUs from the last saved checkpoint,
writes pickle shards, signals NEW_INDEX_READY over gloo, and the trainers reload the 32 GB pickle every --index-reload-interval steps
(train_e2eqa.py:436-508).  MI355X-native form: the index lives row-sharded in the trainers' own HBM (288 GB leaves room for
two images), so each trainer re-embeds ITS rows on a side HIP stream from a frozen snapshot of the context encoder -- the in-process
equivalent of "the checkpoint saved at the last reload" -- packs them into the spare image, and swaps images at a step boundary once the
whole shard is done and the reload interval has passed.  No disk, no host copy, no exchange; the handshake collapses to one barrier.

Usage inside the training loop:

    indexer = AsyncIndexBuilder(model.retriever_model.context_model, arena, index, ...)
    for iteration, batch in enumerate(loader):
        indexer.pump()                         # enqueue a few re-embedding batches on the side stream
        train_step(...)
        indexer.maybe_swap(iteration)          # == NEW_INDEX_READY handling + update_evidence_embedding()

Rolling mode (`in_place=True`, --index-refresh-in-place; not in the reference): no spare image.  What a `pump()` embedded is written into
the image that is being searched at the next step boundary (`index.update_rows`), so the index costs its own size in HBM instead of twice
that, and a row serves weights that are on average one pass old instead of one and a half.  Searches then see a mix of two embedding
generations: a choice of semantics, which is why the atomic swap stays the default.

Snapshots (`--save-index-snapshot`, not in the reference): the reference's indexer group leaves every refreshed index on disk; here it
would exist in HBM only.  With a `snapshot_writer` (data/index_snapshot.IndexSnapshotWriter, driven by train_e2eqa._train) the index just
committed is exported to one flat file, a chunk per step boundary.  A snapshot still open when the next swap is due is finished first
(`maybe_swap`): the image it reads becomes the spare at the swap, and the next pass clears the spare.

Generations (`--index-generations`, not in the reference): on an index that keeps generation stamps every row this builder writes carries
`snapshot_generation`, the number of optimizer steps that were complete when `start()` copied the weights.  The builder is told the step
count at construction (`iteration=`) and by every `maybe_swap(iteration)`; the `pump()` at the top of the loop follows the previous
boundary's `maybe_swap`, so the count it remembers is the right one when a pass ends inside `pump()` and the next snapshot is taken.  Swap
mode stamps the whole spare image once per pass.  Rolling mode queues the generation with every staging tensor -- a pass can end while
earlier batches are still queued -- and with `newest_wins` (--index-newest-wins) a row that holds a newer stamp, a written-back one, is
left alone.

Oldest first (`oldest_first=True`, --index-refresh-oldest-first, not in the reference; rolling mode on a stamped index): the pass has no
row cursor.  Every `pump()` asks the device for the `batches_per_pump * batch_size` OLDEST rows of the shard whose stamp is below the
generation G of the pass's snapshot (`index.oldest_rows`: stamp ascending, row ascending among equal stamps, returned in ascending row
order, -1 in the empty slots), embeds exactly those and queues them for the boundary, where `update_rows_at` writes them.  A row the
write-back has stamped G or later is never selected, so no forward is spent on a row that newest-wins would refuse; a pass ends at the
first boundary whose selection took every eligible row -- no row is then older than the snapshot -- instead of after a fixed count, and
the next `pump()` takes a new snapshot.  Shapes are fixed and `pump()` reads nothing back: the empty slots of a pass's last pump are
embedded with a valid doc id and skipped by the writer (`rows_padded`); the one host read, of the rows selected, is at the boundary,
behind the update's own.  The selection is made from the stamps as the previous boundary's writers left them, so what a boundary writes
is still a function of the step number alone.  On uniform stamps the order is the row order: the sequential pass.
"""
import copy

import torch

from emdr2_amd.indexer_emdr2 import IndexBuilder


PACE_MARGIN = 0.9        # fraction of the reload interval a pass over the shard is paced for


class AsyncIndexBuilder(IndexBuilder):
    def __init__(self, live_context_model, evidence_arena, index, seq_length_ret, cls_id, sep_id, pad_id=0, batch_size=128,
                 log_interval=1000, index_reload_interval=500, batches_per_pump=None, process_group=None, in_place=False, iteration=0,
                 newest_wins=False, oldest_first=False):
        snapshot = copy.deepcopy(live_context_model)
        for p in snapshot.parameters():
            p.requires_grad_(False)
            p.__dict__.pop("_emdr2_cache", None)
            p.__dict__["_emdr2_frozen"] = True                 # bf16 working copies survive the trainer's optimizer steps
        snapshot.eval()
        super().__init__(snapshot, evidence_arena, seq_length_ret, cls_id, sep_id, pad_id, batch_size, log_interval, process_group)
        self.live = live_context_model
        self.index = index
        self.in_place = bool(in_place)
        self.stamped = bool(getattr(index, "generations", False))  # the index keeps generation stamps: every write carries one
        self.newest_wins = bool(newest_wins)
        if self.newest_wins and not (self.stamped and self.in_place):
            raise ValueError("newest_wins needs the rolling mode (in_place) and an index that keeps generation stamps")
        self.oldest_first = bool(oldest_first)
        if self.oldest_first and not (self.stamped and self.in_place):
            raise ValueError("oldest_first needs the rolling mode (in_place) and an index that keeps generation stamps")
        self.steps_done = int(iteration)                        # optimizer steps completed, as last told (construction, maybe_swap)
        self.snapshot_generation = self.steps_done              # ... when start() last copied the weights
        # rolling mode, not yet applied: (first global row, staging rows, event, generation); oldest first: (global rows, staging rows,
        # the selection's report, event, generation)
        self._queued = []
        self.passes = 0                                         # rolling mode: completed passes over the shard
        # oldest first: rows chosen / empty slots embedded for nothing, in all and in the current pass; whether the last boundary ended it
        self.rows_selected = self.rows_padded = 0
        self._pass_selected = self._pass_padded = 0
        self._pass_over = False
        self.snapshot_writer = None                             # --save-index-snapshot: an IndexSnapshotWriter over `index` (train_e2eqa._train)
        self.log = lambda msg: print(msg, flush=True) if self.is_main_builder else None
        self.index_reload_interval = index_reload_interval
        lo, hi = index.local_rows()
        n_batches = (hi - lo + batch_size - 1) // batch_size
        # default pace: finish one pass over the shard within 90 % of a reload interval -- the swap happens at the first step boundary at which
        # EVERY rank's pass is complete (maybe_swap's MIN all-reduce), and ranks do not finish on the same step (the last shard is shorter,
        # side-stream batches queue behind training kernels): a pace that needs 489 of 500 steps (r05) left 2 % for all of that
        paced = max(1, int(index_reload_interval * PACE_MARGIN))
        self.batches_per_pump = batches_per_pump or max(1, (n_batches + paced - 1) // paced)
        self.stream = torch.cuda.Stream()
        self.done_event = None
        self.last_reload_iteration = 0
        self.refreshes = 0
        self._gen = None
        self.start()

    def start(self):
        """Take a new weight snapshot (after everything queued on the training stream) and restart the pass over the shard."""
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            with torch.no_grad():
                for ps, pl in zip(self.model.parameters(), self.live.parameters()):
                    ps.copy_(pl)
                    ps.__dict__.pop("_emdr2_cache", None)
            self.snapshot_generation = self.steps_done
            if self.oldest_first:
                self._gen = None                                # no cursor: every pump asks the device which rows are oldest
            elif self.in_place:
                self._gen = self.embed_batches(self.index)
            else:
                self._gen = self.refresh_batches(self.index, self.snapshot_generation if self.stamped else None)
        self.done_event = None

    def pump(self, n_batches=None):
        """Enqueue up to n re-embedding batches on the side stream; returns True once the whole shard has been enqueued."""
        n = self.batches_per_pump if n_batches is None else n_batches
        if self.in_place:
            return self._pump_in_place(n)
        if self._gen is None:
            return True
        with torch.cuda.stream(self.stream):
            for _ in range(n):
                try:
                    next(self._gen)
                except StopIteration:
                    self._gen = None
                    self.done_event = torch.cuda.Event()
                    self.done_event.record(self.stream)
                    return True
        return False

    def _pump_in_place(self, n):
        """Rolling mode: embed up to n batches on the side stream into ONE contiguous staging tensor and queue it, with an event, for the
        next step boundary.  Returns True when this call reached the end of the shard: the builder has then taken the next weight snapshot
        and restarted at once -- no collective: ranks finish on different steps and need not agree."""
        if self.oldest_first:
            return self._pump_oldest(n)
        lo, hi = self.index.local_rows()
        staging, first, filled, finished = None, None, 0, False
        generation = self.snapshot_generation                   # of the pass these batches belong to: start() below begins the next
        with torch.cuda.stream(self.stream):
            for _ in range(n):
                try:
                    start, emb = next(self._gen)
                except StopIteration:
                    finished = True
                    break
                if staging is None:
                    first = start
                    staging = torch.empty((min(n * self.batch_size, hi - start), emb.shape[1]), dtype=torch.float16, device=emb.device)
                staging[filled:filled + emb.shape[0]].copy_(emb)
                filled += emb.shape[0]
                if start + emb.shape[0] >= hi:
                    finished = True
                    break
            if staging is not None:
                event = torch.cuda.Event()
                event.record(self.stream)
                self._queued.append((first, staging[:filled], event, generation))
        if finished:
            self.passes += 1
            self.start()
        return finished

    def _pump_oldest(self, n):
        """Oldest first: ONE selection of the n * batch_size oldest rows below the pass's generation, on the side stream behind everything
        the current stream has queued (the previous boundary's writers have stored the stamps it reads); their doc ids; their
        embeddings, a batch at a time, into one staging tensor; queued with the selection's report for the next boundary.  Fixed shapes,
        no host read: an empty slot (-1) is embedded with the shard's first doc id and skipped by the writer.  Returns False: that a
        pass has ended is only known at the boundary (`_apply_oldest`), and the call after it takes the next snapshot."""
        if self._pass_over:
            self._pass_over = False
            self.start()
        lo, hi = self.index.local_rows()
        shard = self.index.shard
        generation = self.snapshot_generation
        n_slots = min(n * self.batch_size, hi - lo)
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            rows, info = self.index.oldest_rows(n_slots, below=generation)
            local = (rows - lo).clamp_(min=0)
            doc_ids = shard.ids[local] if shard.ids is not None else (local + (lo + 1)).to(torch.int32)
            staging = torch.empty((n_slots, shard.dim), dtype=torch.float16, device=rows.device)
            for b in range(0, n_slots, self.batch_size):
                emb = self.embed(doc_ids[b:b + self.batch_size])
                staging[b:b + emb.shape[0]].copy_(emb)
                self.track_and_report_progress(batch_size=emb.shape[0])
            event = torch.cuda.Event()
            event.record(self.stream)
            self._queued.append((rows, staging, info, event, generation))
        return False

    def _apply_oldest(self):
        """`_apply_queued` of the oldest-first form: the selected rows go in through the scattered writer, then the selection's report is
        read -- one host read, on a stream the update's own non-finite read-back synchronises anyway.  A selection that took EVERY
        eligible row (always the case when it took fewer than it was asked for) leaves no row older than the pass's snapshot: the pass is
        over.  Returns True when one ended."""
        cur = torch.cuda.current_stream()
        ended = False
        for rows, staging, info, event, generation in self._queued:
            cur.wait_event(event)
            self.index.update_rows_at(rows, staging, generation=generation, newest_wins=self.newest_wins)
            for t in (rows, staging, info):
                t.record_stream(cur)
            n_selected, n_eligible = info[:2].tolist()
            self.rows_selected += n_selected
            self.rows_padded += rows.shape[0] - n_selected
            self._pass_selected += n_selected
            self._pass_padded += rows.shape[0] - n_selected
            if n_selected == n_eligible and not self._pass_over:
                self._pass_over = ended = True
                self.passes += 1
                self.log("oldest-first pass %d complete at iteration %d: %d rows embedded, %d slots padded"
                         % (self.passes, self.steps_done, self._pass_selected, self._pass_padded))
                self._pass_selected = self._pass_padded = 0
        self._queued = []
        return ended

    def _apply_queued(self):
        """At a step boundary: everything pumped so far goes into the live image, in order, on the current stream.  What is applied at a
        step is a function of the step number alone -- never of how far the side stream happens to have got.  Returns True when the
        boundary ended an oldest-first pass."""
        if self.oldest_first:
            return self._apply_oldest()
        cur = torch.cuda.current_stream()
        for first, staging, event, generation in self._queued:
            cur.wait_event(event)                               # the side stream has had the whole step: this rarely waits
            if self.stamped:
                self.index.update_rows(first, staging, generation=generation, newest_wins=self.newest_wins)
            else:
                self.index.update_rows(first, staging)
            staging.record_stream(cur)                          # allocated on the side stream, consumed here: not reused before the update has run
        self._queued = []
        return False

    def ready(self):
        return self._gen is None and self.done_event is not None and self.done_event.query()

    def maybe_swap(self, iteration, force=False):
        """At a step boundary: if the pass is complete (on every rank) and the reload interval has gone by, swap in the new image and
        start the next pass.  Returns True when the index was updated."""
        self.steps_done = int(iteration)                        # (before anything below takes a weight snapshot)
        if self.in_place:
            # Rolling mode.  The rows go in at EVERY boundary; the return value keeps the reference's cadence on the rank-uniform interval
            # condition alone (the training loop logs and checkpoints on it: a collective save cannot be entered by some ranks only).
            self._apply_queued()
            while force:                                        # drain the current pass, a pump at a time (the staging tensor stays small)
                done = self._pump_in_place(self.batches_per_pump)
                done = self._apply_queued() or done             # (oldest first: the boundary, not the pump, finds the pass over)
                if done:
                    break
            if not force and iteration < self.last_reload_iteration + self.index_reload_interval:
                return False
            self.refreshes += 1
            self.last_reload_iteration = iteration
            return True
        # Only rank-uniform conditions may return before the collective below: `iteration`, `force` and the interval are the same on every
        # rank, the state of this rank's pass is not (the last shard is shorter, so ranks finish their passes on different steps).
        if not force and iteration < self.last_reload_iteration + self.index_reload_interval:
            return False
        if force:
            while not self.pump(1 << 30):
                pass
        flag = torch.tensor([1 if (force or (self._gen is None and self.ready())) else 0], dtype=torch.int32, device="cuda")
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN, group=self.process_group)
        if int(flag.item()) == 0:
            return False
        torch.cuda.current_stream().wait_event(self.done_event)        # searches after this point see the finished image
        writer = self.snapshot_writer
        if writer is not None and writer.active:
            # (rank-uniform: a snapshot begins and ends in collectives.)  The image being exported becomes the spare at the swap and the
            # next pass clears it: what is left of the snapshot is written now, at the cost of one slow step
            self.log("Training Group: finishing the open index snapshot before the swap at iteration {}".format(iteration))
            writer.finish()
        self.index.commit_refresh()
        self.refreshes += 1
        self.last_reload_iteration = iteration
        self.start()
        return True
