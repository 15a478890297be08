"""Time emdr2_answer_hits against emdr2_assemble_evidence -- the launch that reads the same passages and writes far more -- on the same doc
ids, in one process, alternating the two (profiles/answer_hits.txt).

  python tools/answer_hits_bench.py [--out FILE] [--docs N]

Shapes: B = 64 questions x K = 50 and K = 100 retrieved passages on `EvidenceArena.synthetic`; 1, 16 and 256 answers per question, each of 1-8
tokens, half of them sharing one first token.  Device events around blocks of back-to-back launches (time per launch = block / launches) and
around single launches; medians over alternating repetitions.  Also the host time to pack one batch's answers from strings, uncached."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from emdr2_amd import _native  # noqa: E402
from emdr2_amd.data.answer_match import AnswerPack, _to_device, pack_answers  # noqa: E402
from emdr2_amd.data.evidence_arena import EvidenceArena  # noqa: E402

BLOCK, REPS, SINGLES, VOCAB = 20, 30, 200, 30522


def token_pack(rng, n_q, n_ans):
    """n_ans answers per question of 1-8 tokens; every second answer of a question starts with the question's shared first token."""
    tokens, ans_off, q_ans_off = [], [0], [0]
    for _ in range(n_q):
        shared = int(rng.integers(5, VOCAB))
        for a in range(n_ans):
            t = rng.integers(5, VOCAB, size=int(rng.integers(1, 9))).tolist()
            if a % 2:
                t[0] = shared
            tokens.extend(t)
            ans_off.append(len(tokens))
        q_ans_off.append(len(ans_off) - 1)
    return AnswerPack(np.asarray(tokens, np.uint16), np.asarray(ans_off, np.int32), np.asarray(q_ans_off, np.int32),
                      np.zeros(len(ans_off) - 1, np.int32), 0)


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / launches          # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--docs", type=int, default=2_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("answer_hits_bench needs a GPU: there is nothing to measure without one")
    lib, stream = _native.lib(), _native.stream_ptr()
    rng = np.random.default_rng(0)
    arena = EvidenceArena.synthetic(args.docs, seed=1)
    cont = np.zeros(2048, np.uint32)
    for t in range(0, 65536, 4):                            # a quarter of the vocabulary are continuation pieces
        cont[t >> 5] |= np.uint32(1 << (t & 31))
    d_cont = _to_device(cont, "cuda")
    lines = ["answer hits vs evidence assembly, %s, %d synthetic passages (%.0f MB of token ids), B = 64, S = 512, S_ret = 256"
             % (torch.cuda.get_device_name(0), args.docs, arena.dev["passage_tokens"].numel() * 2 / 1e6),
             "us per launch: median of %d alternating blocks of %d back-to-back launches [min .. max], and median of %d single launches"
             % (REPS, BLOCK, SINGLES), ""]
    B = 64
    for K in (50, 100):
        ids = torch.from_numpy(rng.integers(1, args.docs + 1, size=(B, K + 1)).astype(np.int32)).cuda()
        uid = -torch.arange(1, B + 1, dtype=torch.int64, device="cuda")
        q = torch.randint(5, VOCAB, (B, 64), dtype=torch.int64, device="cuda")
        ql = torch.randint(8, 33, (B,), dtype=torch.int64, device="cuda")
        ctx = torch.empty((B, K, 256), dtype=torch.int64, device="cuda"); typ = torch.empty_like(ctx)
        ext = torch.empty((B * K, 512), dtype=torch.int64, device="cuda"); one = torch.empty_like(ext)
        kept = torch.empty((B, K), dtype=torch.int32, device="cuda")

        def assemble():
            _native.check(lib.emdr2_assemble_evidence(ctypes.byref(arena._struct), ids.data_ptr(), B, K + 1, K, uid.data_ptr(), q.data_ptr(), 64,
                                                      ql.data_ptr(), 256, 512, 101, 102, 0, ctx.data_ptr(), typ.data_ptr(), ext.data_ptr(),
                                                      one.data_ptr(), kept.data_ptr(), stream), "assemble")
        assemble()
        hit_pos = torch.empty((B, K), dtype=torch.int32, device="cuda"); hit_ans = torch.empty_like(hit_pos)
        best = torch.empty((B,), dtype=torch.int32, device="cuda")
        hist = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
        for n_ans in (1, 16, 256):
            pack = token_pack(rng, B, n_ans)
            d_tok, d_off, d_qoff = _to_device(pack.tokens, "cuda"), _to_device(pack.ans_off, "cuda"), _to_device(pack.q_ans_off, "cuda")

            def hits():
                _native.check(lib.emdr2_answer_hits(ctypes.byref(arena._struct), kept.data_ptr(), B, K, d_tok.data_ptr(), d_off.data_ptr(),
                                                    d_qoff.data_ptr(), d_cont.data_ptr(), hit_pos.data_ptr(), hit_ans.data_ptr(),
                                                    best.data_ptr(), hist.data_ptr(), stream), "answer_hits")
            for fn in (assemble, hits):
                timed(fn, BLOCK)
            res = {"assemble": [], "hits": []}
            for _ in range(REPS):
                res["assemble"].append(timed(assemble, BLOCK))
                res["hits"].append(timed(hits, BLOCK))
            single = {"assemble": [], "hits": []}
            for _ in range(SINGLES):
                single["assemble"].append(timed(assemble, 1))
                single["hits"].append(timed(hits, 1))
            n_hit = int((hit_pos >= 0).sum())
            row = "K = %3d  answers/question = %3d (%6d answer tokens, %d of %d pairs hit):" % (K, n_ans, len(pack.tokens), n_hit, B * K)
            for name in ("assemble", "hits"):
                r = res[name]
                row += "  %s %.1f [%.1f .. %.1f] single %.1f" % (name, statistics.median(r), min(r), max(r), statistics.median(single[name]))
            row += "  hits/assemble %.2f" % (statistics.median(res["hits"]) / statistics.median(res["assemble"]))
            lines.append(row)
            print(row, flush=True)
    # host packing of one batch from strings (uncached; the task caches it per question)
    from emdr2_amd.tokenizer import BertWordPieceTokenizer
    tok = BertWordPieceTokenizer(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab.txt"))
    words = [w for w in tok.vocab if w.isalpha()]
    lines.append("")
    for n_ans in (1, 16, 256):
        lists = [[" ".join(rng.choice(words, size=int(rng.integers(1, 9)))) for _ in range(n_ans)] for _ in range(B)]
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            pack_answers(lists, tok)
            t.append((time.perf_counter() - t0) * 1000.0)
        lines.append("host pack_answers, 64 questions x %3d answers of 1-8 words, uncached: %.2f ms per batch (median of 5)" % (n_ans, statistics.median(t)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
