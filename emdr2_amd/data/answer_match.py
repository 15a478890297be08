"""Answer hits on the device (include/emdr2_answers.h): which retrieved passages hold a reference answer, matched on the WordPiece ids of
the evidence arena instead of on the evidence text (reference: tasks/openqa/dense_retriever/evaluation/qa_validation.py:29-125).

  continuation_bits(tokenizer)   the `##` pieces of the vocabulary as the kernel's bitset
  pack_answers(lists, tokenizer) the answers of a batch of questions, tokenised and laid out for the kernel (host work, cacheable:
                                 `concat_packs` joins the packs of single questions)
  AnswerMatcher(arena, tok)      .hits(doc_ids, pack) -> (hit_pos, hit_ans, best_slot) device tensors, one launch pair, no host read
  HitMeter(k)                    the histogram of best slots and the question count; .report(ks) -> hits@k counts

The matching rule, and where it differs from the reference's string matcher (CJK runs, answers with [UNK]), is stated in the header.
There is no CPU fallback: without a GPU `AnswerMatcher` raises NativeError, like `EvidenceArena.to_device`."""
import collections
import ctypes

import numpy as np
import torch

from emdr2_amd import _native

CONT_WORDS = 2048                                         # 65,536 token ids, one bit each

AnswerPack = collections.namedtuple("AnswerPack", ["tokens", "ans_off", "q_ans_off", "orig", "dropped"])
AnswerPack.__doc__ = """tokens u16: all answers' ids; ans_off i32: answer a = tokens[ans_off[a]:ans_off[a + 1]]; q_ans_off i32 [B + 1]: question b
owns the answers q_ans_off[b]:q_ans_off[b + 1]; orig i32: a packed answer's index in its question's own list; dropped: answers left out
because their tokenisation holds [UNK]."""


def continuation_bits(tokenizer):
    """np.uint32[2048]: bit t set = vocabulary entry t starts with `##` (a word-internal piece).  Ids beyond uint16 cannot occur in the arena."""
    bits = np.zeros(CONT_WORDS, dtype=np.uint32)
    for i, tok in tokenizer.inv_vocab.items():
        if 0 <= int(i) < 65536 and tok.startswith("##"):
            bits[int(i) >> 5] |= np.uint32(1 << (int(i) & 31))
    return bits


def pack_answers(answer_lists, tokenizer):
    """answer_lists: one list of answer strings per question -> AnswerPack.  An answer with [UNK] is dropped (it would match any unknown
    word); an answer that tokenises to nothing is kept (it occurs in every passage, as in the reference)."""
    unk = tokenizer.vocab.get("[UNK]")
    tokens, ans_off, q_ans_off, orig, dropped = [], [0], [0], [], 0
    for answers in answer_lists:
        for i, answer in enumerate(answers):
            ids = [int(t) for t in tokenizer.tokenize(answer)]
            if unk is not None and unk in ids:
                dropped += 1
                continue
            if ids and (min(ids) < 0 or max(ids) > 65535):
                raise ValueError("token ids must fit uint16")
            tokens.extend(ids)
            ans_off.append(len(tokens))
            orig.append(i)
        q_ans_off.append(len(ans_off) - 1)
    return AnswerPack(np.asarray(tokens, dtype=np.uint16), np.asarray(ans_off, dtype=np.int32), np.asarray(q_ans_off, dtype=np.int32),
                      np.asarray(orig, dtype=np.int32), dropped)


def concat_packs(packs):
    """The pack of a batch from the packs of its questions (e.g. single-question packs cached by query uid), in order."""
    tokens = np.concatenate([p.tokens for p in packs]) if packs else np.zeros(0, dtype=np.uint16)
    ans_off, q_ans_off, t_at, a_at = [np.zeros(1, dtype=np.int32)], [np.zeros(1, dtype=np.int32)], 0, 0
    for p in packs:
        ans_off.append(p.ans_off[1:] + t_at)
        q_ans_off.append(p.q_ans_off[1:] + a_at)
        t_at += int(p.ans_off[-1])
        a_at += int(p.q_ans_off[-1])
    orig = np.concatenate([p.orig for p in packs]) if packs else np.zeros(0, dtype=np.int32)
    return AnswerPack(tokens.astype(np.uint16), np.concatenate(ans_off).astype(np.int32), np.concatenate(q_ans_off).astype(np.int32),
                      orig.astype(np.int32), sum(p.dropped for p in packs))


def _to_device(a, dev):
    """A host table on the device; never an empty allocation (its pointer would be null)."""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, dtype=a.dtype)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view is not None else a).to(dev)


class AnswerMatcher(object):
    def __init__(self, arena, tokenizer):
        """arena: an EvidenceArena (moved to the device if it is not there); tokenizer: the one the arena's passages were tokenised with."""
        if not torch.cuda.is_available():
            raise _native.NativeError("AnswerMatcher needs a GPU; there is no CPU fallback")
        if arena._struct is None:
            arena.to_device()
        self.arena = arena
        self.device = arena.dev["passage_tokens"].device
        self.cont_bits = _to_device(continuation_bits(tokenizer), self.device) if tokenizer is not None else None

    def hits(self, doc_ids, pack, hist=None):
        """doc_ids: integer device tensor [B, K] (1-based; e.g. the kept ids of `EvidenceArena.assemble`); pack: the AnswerPack of the same
        B questions; hist: int64 device tensor [K + 1] the best slots are counted INTO, or None.
        -> (hit_pos [B, K], hit_ans [B, K], best_slot [B]) int32 on the device; no host synchronisation."""
        if not torch.is_tensor(doc_ids) or not doc_ids.is_cuda or doc_ids.device != self.device:
            raise TypeError("doc_ids must be a tensor on the arena's device (%s)" % (self.device,))
        if doc_ids.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
            raise TypeError("doc_ids must hold integers (got %s)" % (doc_ids.dtype,))
        if doc_ids.dim() != 2 or doc_ids.shape[0] < 1 or doc_ids.shape[1] < 1:
            raise ValueError("doc_ids must be [B, K] with B, K >= 1 (got %s)" % (tuple(doc_ids.shape),))
        b, k = doc_ids.shape
        if len(pack.q_ans_off) != b + 1:
            raise ValueError("the answer pack holds %d questions, doc_ids %d" % (len(pack.q_ans_off) - 1, b))
        if doc_ids.dtype == torch.int64:
            doc_ids = doc_ids.clamp(-1, 2 ** 31 - 1)                      # (an id beyond int32 is beyond n_docs: no hit either way)
        ids = doc_ids.to(torch.int32).contiguous()
        if hist is not None:
            if not torch.is_tensor(hist) or hist.device != self.device or hist.dtype != torch.int64 or not hist.is_contiguous():
                raise TypeError("hist must be a contiguous int64 tensor on the arena's device")
            if tuple(hist.shape) != (k + 1,):
                raise ValueError("hist must have K + 1 = %d bins (got %s)" % (k + 1, tuple(hist.shape)))
        dev = self.device
        tokens, ans_off, q_ans_off = _to_device(pack.tokens, dev), _to_device(pack.ans_off, dev), _to_device(pack.q_ans_off, dev)
        hit_pos = torch.empty((b, k), dtype=torch.int32, device=dev)
        hit_ans = torch.empty_like(hit_pos)
        best = torch.empty((b,), dtype=torch.int32, device=dev)
        _native.check(_native.lib().emdr2_answer_hits(
            ctypes.byref(self.arena._struct), ids.data_ptr(), b, k, tokens.data_ptr(), ans_off.data_ptr(), q_ans_off.data_ptr(),
            self.cont_bits.data_ptr() if self.cont_bits is not None else None, hit_pos.data_ptr(), hit_ans.data_ptr(), best.data_ptr(),
            hist.data_ptr() if hist is not None else None, _native.stream_ptr()), "answer_hits")
        return hit_pos, hit_ans, best


class HitMeter(object):
    """The histogram of best slots (k + 1 bins, bin k = no hit) and the number of questions behind it.  `hist` lives on `device` and is
    what `AnswerMatcher.hits(..., hist=meter.hist)` adds into."""

    def __init__(self, k, device=None):
        self.k = int(k)
        self.hist = torch.zeros(self.k + 1, dtype=torch.int64, device=device)
        self.count = 0

    def update(self, best_slot=None, n=None):
        """Count a batch of questions; no host read.  `best_slot` [B]: added into the histogram here; None: the kernel has already added
        them (`hist=meter.hist`) and `n` says how many questions that was."""
        if best_slot is not None:
            self.hist.index_add_(0, best_slot.to(torch.int64), torch.ones_like(best_slot, dtype=torch.int64))
            n = best_slot.numel()
        self.count += int(n)

    def report(self, ks, group=None):
        """-> {k: number of questions with a hit among their first k slots for k in ks, 'total': questions}, summed over the ranks of
        `group` when torch.distributed is initialised (one int64 all-reduce), read in one host transfer; the meter starts again at zero.
        The reference's top_k_hits[k - 1] (qa_validation.py:65-72) is the same prefix sum."""
        packed = torch.cat([self.hist, torch.tensor([self.count], dtype=torch.int64).to(self.hist.device)])
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(packed, group=group)
        vals = packed.tolist()
        out = {int(k): int(sum(vals[:min(int(k), self.k)])) for k in ks}
        out["total"] = int(vals[-1])
        self.hist.zero_()
        self.count = 0
        return out
