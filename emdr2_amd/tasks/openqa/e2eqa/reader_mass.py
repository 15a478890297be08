"""--reader-attention-mass: which of the retrieved passages the FiD decoder reads.  The model leaves, per question, the decoder's
cross-attention probability mass on each of its K passage slots (`EMDR2Model.last_attention_mass`, csrc/attention_mass.hip); this meter
turns it into the numbers of the training log line, next to `AnswerHitTracker` and with its protocol: the forward step calls `begin`,
the model calls `add` per question group, the training loop `commit` when the step is done -- a step that is run again after an
allocation failure is counted once -- and `line` at every --log-interval.  Nothing is read on the host before `line`.

    read entropy        mean entropy (nats) of the per-question distribution over the K slots: ln K = the decoder does not choose
    read-prior agree    questions whose most-read slot is the slot the retriever's prior ranks first
    read mass           (with --retrieval-answer-hits) mean attention mass on answer-bearing slots: comparable to `hit mass`
    read top1 hit       (with --retrieval-answer-hits) questions whose most-read slot holds an answer

A question without a weighted decoder position has an all-zero row and is not counted."""
import torch

NAMES = ("questions", "entropy", "agree", "hit_mass", "top1_hit")


def mass_statistics(mass, topk_log_probs, hits=None):
    """mass fp32 [B, K] (rows sum to 1, or are all zero), the prior's log-probabilities [B, K], hits bool [B, K] or None ->
    fp64 [5] sums in the order of NAMES: counted questions, their entropies, prior agreements, mass on hit slots, top-1 hits."""
    mass = mass.detach().double()
    live = mass.sum(dim=1) > 0
    plogp = torch.where(mass > 0, mass * torch.log(torch.where(mass > 0, mass, torch.ones_like(mass))), torch.zeros_like(mass))
    top = mass.argmax(dim=1)
    agree = top == topk_log_probs.detach().float().argmax(dim=1)
    out = [live.sum(), -(plogp.sum(dim=1) * live).sum(), (agree & live).sum()]
    if hits is not None:
        hits = hits.to(torch.bool)
        out += [(mass * hits).sum(), (hits.gather(1, top[:, None])[:, 0] & live).sum()]
    else:
        out += [torch.zeros((), device=mass.device), torch.zeros((), device=mass.device)]
    return torch.stack([v.double() for v in out])


class ReaderMassMeter(object):
    def __init__(self, topk, tracker=None):
        """tracker: the model's AnswerHitTracker (--retrieval-answer-hits) or None; its hit slots of the step are read at `add`."""
        self.topk, self.tracker = int(topk), tracker
        self.total = self._step = None
        self._armed = False

    def begin(self):
        """Start of a step's forward; whatever an unfinished step left is dropped."""
        self._step, self._armed = None, True

    def add(self, mass, topk_log_probs, lo, hi, hits=None):
        """The questions lo..hi of the step: their attention mass [hi - lo, K] and prior.  A no-op unless `begin` armed it."""
        if not self._armed or mass is None:
            return
        if hits is None and self.tracker is not None and self.tracker._step_hits is not None:
            hits = self.tracker._step_hits[lo:hi]
        s = mass_statistics(mass, topk_log_probs, hits)
        self._step = s if self._step is None else self._step + s

    def commit(self):
        if self._step is not None:
            self.total = self._step if self.total is None else self.total + self._step
        self._step, self._armed = None, False

    def line(self, group=None):
        """The part of the --log-interval line, over the questions since the last line, all ranks' summed."""
        with_hits = self.tracker is not None
        if self.total is None:
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
            self.total = torch.zeros(len(NAMES), dtype=torch.float64, device=dev)
        total = self.total.clone()
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(total, group=group)
        self.total = None
        n, ent, agree, hit_mass, top1 = total.tolist()
        n = int(round(n))
        out = " read entropy: {:.4f} | read-prior agree: {}/{} |".format(ent / max(n, 1), int(round(agree)), n)
        if with_hits:
            out += " read mass: {:.4f} | read top1 hit: {}/{} |".format(hit_mass / max(n, 1), int(round(top1)), n)
        return out
