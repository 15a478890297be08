"""--retrieval-answer-hits: how often, and at which rank, the passages the reader is shown hold a reference answer -- the number the
reference reports through its separate retrieval evaluator (tasks/openqa/dense_retriever/evaluation/evaluate.py:42-164), taken here
from the passages each training step and each evaluation batch has retrieved anyway, on the device (emdr2_amd/data/answer_match.py).

Training: the forward step hands the batch's reference answers to `begin`; the model calls `match` once per step, right after the
search and the evidence assembly (one launch pair on the kept ids, whatever --question-micro-batches says), and `add_mass` per question
group with that group's prior; the training loop calls `commit` when the step is done -- a step that is run again after an allocation
failure is counted once -- and `line` at every --log-interval.  Evaluation: `reader_em_score` calls `best_slots`."""
import torch

from emdr2_amd.data.answer_match import AnswerMatcher, HitMeter, concat_packs, pack_answers


def report_ranks(report_topk_accuracies, topk):
    """The ranks reported: --report-topk-accuracies cut to <= --topk-retrievals; 1 5 20 <topk> when that list is empty."""
    ks = list(report_topk_accuracies) if report_topk_accuracies else [1, 5, 20, topk]
    return sorted({int(k) for k in ks if 1 <= int(k) <= topk})


class AnswerHitTracker(object):
    def __init__(self, arena, tokenizer, topk, ks):
        self.matcher = AnswerMatcher(arena, tokenizer)
        self.tokenizer, self.topk, self.ks = tokenizer, int(topk), list(ks)
        dev = self.matcher.device
        self.meter = HitMeter(self.topk, device=dev)
        self.mass = torch.zeros((), dtype=torch.float32, device=dev)          # the retriever's probability mass on hit slots, summed
        self._packs = {}                                                       # (query uid, answers) -> their pack (tokenised once)
        self._pending = None
        self._step_hist = torch.zeros(self.topk + 1, dtype=torch.int64, device=dev)
        self._step_mass = torch.zeros_like(self.mass)
        self._step_hits, self._step_n = None, 0

    def pack(self, query_uids, references):
        packs = []
        for uid, answers in zip(query_uids, references):
            key = (uid, tuple(answers))                                        # (uids repeat across the training and evaluation files)
            p = self._packs.get(key)
            if p is None:
                p = self._packs[key] = pack_answers([answers], self.tokenizer)
            packs.append(p)
        return concat_packs(packs)

    # ---- training --------------------------------------------------------------------------------------------------------------------
    def begin(self, query_uids, references):
        """Start of a step's forward: the answers the step's retrieval will be matched against.  Whatever an unfinished step left is dropped."""
        self._pending = self.pack(query_uids, references)
        self._step_hist.zero_()
        self._step_mass.zero_()
        self._step_hits, self._step_n = None, 0

    def match(self, kept_ids):
        """Once per step, on the doc ids the reader is shown [B, K]; a no-op unless `begin` has armed it (evaluation-mode forwards)."""
        if self._pending is None:
            return
        pack, self._pending = self._pending, None
        self._step_hits = self.matcher.hits(kept_ids, pack, hist=self._step_hist)[0] >= 0
        self._step_n = kept_ids.shape[0]

    def add_mass(self, topk_log_probs, lo, hi):
        """The prior [hi - lo, K] of the questions lo..hi of the step: its mass on their hit slots."""
        if self._step_hits is not None:
            self._step_mass += (torch.exp(topk_log_probs.detach().float()) * self._step_hits[lo:hi]).sum()

    def commit(self):
        """The step is done: count it.  No host read."""
        if self._step_hits is None:
            return
        self.meter.hist += self._step_hist
        self.meter.update(n=self._step_n)
        self.mass += self._step_mass
        self._step_hits, self._step_n = None, 0

    def line(self, group=None):
        """The part of the --log-interval line: hits@k of the questions since the last line, all ranks' summed, and the mean hit mass."""
        mass = self.mass.clone()
        rep = self.meter.report(self.ks, group)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(mass, group=group)
        self.mass.zero_()
        total = rep["total"]
        out = "".join(" answer hits@{}: {}/{} |".format(k, rep[k], total) for k in self.ks)
        return out + " hit mass: {:.4f} |".format(float(mass) / max(total, 1))

    # ---- evaluation ------------------------------------------------------------------------------------------------------------------
    def best_slots(self, query_uids, references, kept_ids):
        """-> (hit_pos [B, K], best_slot [B]) device tensors of an evaluation batch; the training meter is not touched."""
        hit_pos, _, best = self.matcher.hits(kept_ids, self.pack(query_uids, references))
        return hit_pos, best


def answer_hit_table(model, dataloader):
    """For tests and inspection: every question of `dataloader` through the model's retrieval in evaluation mode (no decoding) ->
    [{'uid', 'answers', 'kept_ids' [K], 'hit_pos' [K], 'best_slot'}], in data order."""
    from emdr2_amd.tasks.openqa.e2eqa.train_e2eqa import process_batch
    tracker = model.answer_hits
    if tracker is None:
        raise RuntimeError("the model was built without --retrieval-answer-hits")
    rows, was_training = [], model.training
    model.eval()
    with torch.no_grad():
        for batch in dataloader:
            query_uid, q_bert, q_types, q_mask, q_t5, q_t5_len, _, _, _, reference = process_batch(batch)
            model(query_uid, q_bert, q_types, q_mask, q_t5, q_t5_len, None)
            kept = model.evidence_retriever.last_kept_ids
            hit_pos, best = tracker.best_slots(query_uid.tolist(), reference, kept)
            for uid, ans, ids, pos, b in zip(query_uid.tolist(), reference, kept.tolist(), hit_pos.tolist(), best.tolist()):
                rows.append({"uid": uid, "answers": list(ans), "kept_ids": ids, "hit_pos": pos, "best_slot": b})
    model.train(was_training)
    return rows
