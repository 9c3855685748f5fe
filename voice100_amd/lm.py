"""A back-off n-gram language model over the acoustic model's own label ids, for the fused CTC prefix beam search (K25,
decode.ctc_beam_search(lm=...)).  Characters or phones: the space is a label like any other, so there is no lexicon and no word level.

The model is the ARPA one: per order n a table {n-gram: (log p(last | the rest), back-off weight of the whole n-gram)}, natural log in
float64, and
    p(c | h) = the value of h + (c,) where it is listed, else bow(h) * p(c | h[1:])          (bow(h) = 1 where h is not listed)
on the last N - 1 tokens of the history.  Tokens are the label ids 0 .. V - 1 (never the blank) and two more, NGramLM.bos = V for
<s> and NGramLM.eos = V + 1 for </s>.  `ngrams[n - 1]` is the table of order n, keyed by tuples of tokens.

from_arpa reads the text format, fit estimates a small model from id sequences (nothing here needs an LM toolkit), to_arpa writes the
text back, and compile() resolves the back-off into a deterministic automaton, the form the kernel reads:
    states        the empty context and every listed n-gram of order < N that does not end in </s>
    logp [S, V]   float32, log p(c | state); the blank column holds 0 and never enters a result
    next [S, V]   int32, the longest suffix of state + (c,) that is a state; the blank column holds the state itself
    final [S]     float32, log p(</s> | state), 0 where the model has no </s>
    start         the state of (<s>,) where the model has <s>, else the empty context
Table size: S V (4 + 4) bytes for the two tables; a character 5-gram of 10^5 contexts at V = 29 is 23 MB.  S V <= 2^28 is the limit.
compile() is Python over the states with numpy rows: seconds for 10^5 contexts."""
import math
import os

import numpy as np
import torch

__all__ = ["NGramLM"]

MAX_ORDER = 8
MAX_CELLS = 1 << 28
_LN10 = math.log(10.0)


class NGramLM:
    def __init__(self, vocab_size, order, ngrams, blank=0, symbols=None):
        self.vocab_size, self.order, self.blank = int(vocab_size), int(order), int(blank)
        self.bos, self.eos = self.vocab_size, self.vocab_size + 1
        self.ngrams = ngrams                             # [order] of {tuple of tokens: (logp, bow)}; None for from_tables
        self.symbols = list(symbols) if symbols is not None else None
        self.has_bos = ngrams is not None and (self.bos,) in ngrams[0]
        self.has_eos = ngrams is not None and (self.eos,) in ngrams[0]
        self.logp = self.next = self.final = None        # compile()
        self.start, self.states = 0, None

    # ---- the model as a function of the history ---------------------------------------------------------------------------------
    def start_history(self):
        return (self.bos,) if self.has_bos else ()

    def _lookup(self, history, tok):
        ctx = tuple(history)[-(self.order - 1):] if self.order > 1 else ()
        acc = 0.0
        while True:
            hit = self.ngrams[len(ctx)].get(ctx + (tok,))
            if hit is not None:
                return acc + hit[0]
            if not ctx:
                return -math.inf
            own = self.ngrams[len(ctx) - 1].get(ctx)
            if own is not None:
                acc += own[1]
            ctx = ctx[1:]

    def log_prob(self, history, label):
        """log p(label | history): the back-off walk over the tables; history = start_history() + the labels so far."""
        return self._lookup(history, int(label))

    def log_prob_eos(self, history):
        """log p(</s> | history), 0 where the model has no </s>."""
        return self._lookup(history, self.eos) if self.has_eos else 0.0

    # ---- ARPA text ------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arpa(cls, path_or_text, symbols, blank=0, unk_logp=None):
        """The standard text format.  symbols: the V strings id -> LM token (the entry at `blank` is ignored).  <s> and </s> are
        recognised; n-grams with any other token that is not a symbol (<unk> among them) are skipped.  A non-blank symbol without a
        unigram takes the <unk> entry's probability, else unk_logp (natural log), else ValueError.  Malformed text: ValueError with
        the line number."""
        text = str(path_or_text)
        if "\n" not in text and "\\data\\" not in text:
            with open(os.fspath(path_or_text)) as f:
                text = f.read()
        V = len(symbols)
        bos, eos = V, V + 1
        tok = {s: i for i, s in enumerate(symbols) if i != blank}
        tok["<s>"], tok["</s>"] = bos, eos

        def bad(no, what):
            return ValueError(f"ARPA line {no}: {what}")

        counts, tables, unk = {}, [], None
        section, seen, phase, ended = 0, 0, "head", False
        lines = text.split("\n")
        no = 0

        def close(no):
            if section and seen != counts[section]:
                raise bad(no, f"{seen} {section}-grams where the header announces {counts[section]}")

        for no, raw in enumerate(lines, 1):
            line = raw.strip()
            if not line:
                continue
            if ended:
                raise bad(no, "text after \\end\\")
            if phase == "head":
                if line != "\\data\\":
                    raise bad(no, "\\data\\ expected")
                phase = "counts"
            elif line == "\\end\\":
                close(no)
                if section != len(counts) or not counts:
                    raise bad(no, f"\\end\\ after {section} of {len(counts)} sections")
                ended = True
            elif line.startswith("\\") and line.endswith("-grams:"):
                close(no)
                try:
                    n = int(line[1:-7])
                except ValueError:
                    raise bad(no, f"bad section header {line!r}") from None
                if n != section + 1 or n not in counts:
                    raise bad(no, f"section {n} where {section + 1} of {len(counts)} is expected")
                section, seen, phase = n, 0, "grams"
                tables.append({})
            elif phase == "counts":
                if not line.startswith("ngram ") or "=" not in line:
                    raise bad(no, f"'ngram N=count' expected, got {line!r}")
                try:
                    n, c = (int(x) for x in line[6:].split("="))
                except ValueError:
                    raise bad(no, f"'ngram N=count' expected, got {line!r}") from None
                if n != len(counts) + 1 or c < 0:
                    raise bad(no, f"order {n} where {len(counts) + 1} is expected")
                if n > MAX_ORDER:
                    raise bad(no, f"order {n} is above the limit of {MAX_ORDER}")
                counts[n] = c
            else:
                parts = line.split()
                if len(parts) not in (section + 1, section + 2):
                    raise bad(no, f"a {section}-gram has {section} tokens after the probability and at most one back-off weight")
                try:
                    lp = float(parts[0]) * _LN10
                    bow = float(parts[section + 1]) * _LN10 if len(parts) == section + 2 else 0.0
                except ValueError:
                    raise bad(no, f"not a number in {line!r}") from None
                if math.isnan(lp) or math.isnan(bow) or lp > 1e-6:
                    raise bad(no, f"not a log probability in {line!r}")
                seen += 1
                words = parts[1:section + 1]
                if section == 1 and words[0] == "<unk>":
                    unk = lp
                if any(w not in tok for w in words):
                    continue
                g = tuple(tok[w] for w in words)
                if g in tables[-1]:
                    raise bad(no, f"{' '.join(words)!r} is listed twice")
                if section > 1 and g[:-1] not in tables[-2]:
                    raise bad(no, f"the context of {' '.join(words)!r} is not among the {section - 1}-grams")
                tables[-1][g] = (lp, bow)
        if not ended:
            raise bad(no, "\\end\\ is missing")
        fill = unk if unk is not None else unk_logp
        for i, s in enumerate(symbols):
            if i != blank and (i,) not in tables[0]:
                if fill is None:
                    raise ValueError(f"symbol {s!r} (id {i}) is not among the unigrams, and there is neither <unk> nor unk_logp")
                tables[0][(i,)] = (float(fill), 0.0)
        return cls(V, len(tables), tables, blank, symbols)

    def to_arpa(self, symbols=None):
        """The model as ARPA text (log10, 9 decimals: 2.3e-9 in natural log).  symbols default to those it was read with, else the ids
        as decimal strings."""
        if self.ngrams is None:
            raise ValueError("to_arpa: this model has no n-gram tables (it was built from automaton tables)")
        symbols = symbols if symbols is not None else self.symbols
        name = {i: (str(i) if symbols is None else symbols[i]) for i in range(self.vocab_size)}
        name[self.bos], name[self.eos] = "<s>", "</s>"
        out = ["\\data\\"] + [f"ngram {n + 1}={len(t)}" for n, t in enumerate(self.ngrams)]
        for n, table in enumerate(self.ngrams):
            out += ["", f"\\{n + 1}-grams:"]
            for g in sorted(table):
                lp, bow = table[g]
                row = f"{max(lp / _LN10, -99.0):.9f}\t" + " ".join(name[t] for t in g)
                if n + 1 < self.order and g[-1] != self.eos:
                    row += f"\t{bow / _LN10:.9f}"
                out.append(row)
        return "\n".join(out + ["", "\\end\\", ""])

    # ---- a small estimator ----------------------------------------------------------------------------------------------------------
    @classmethod
    def fit(cls, sequences, vocab_size, order, blank=0, discount=0.75):
        """Interpolated absolute discounting with one discount D on raw counts, float64: with c(h) = sum_w c(h, w) and N(h) = the number
        of different w after h,
            p(w | h) = max(c(h, w) - D, 0) / c(h) + D N(h) / c(h) * p(w | h[1:]),      p(w | nothing before order 1) = 1 / V
        over w in the V - 1 non-blank labels and </s>.  Every sequence of ids is counted as <s> ids </s>.  The tables hold p(w | h) for
        the n-grams seen and bow(h) = D N(h) / c(h), so the back-off walk gives exactly the formula and every context sums to 1."""
        V, N = int(vocab_size), int(order)
        if not 1 <= N <= MAX_ORDER or V < 2 or not 0 <= blank < V or not 0.0 < discount < 1.0:
            raise ValueError(f"fit: 1 <= order <= {MAX_ORDER}, vocab_size >= 2, 0 <= blank < vocab_size and 0 < discount < 1 are required")
        bos, eos = V, V + 1
        cnt = [{} for _ in range(N)]
        for seq in sequences:
            seq = [int(x) for x in seq]
            if any(not 0 <= x < V or x == blank for x in seq):
                raise ValueError("fit: ids must be non-blank labels in [0, vocab_size)")
            s = [bos] + seq + [eos]
            for n in range(1, N + 1):
                for i in range(0 if n > 1 else 1, len(s) - n + 1):      # <s> is never predicted: no unigram count
                    g = tuple(s[i:i + n])
                    cnt[n - 1][g] = cnt[n - 1].get(g, 0) + 1
        if not cnt[0]:
            raise ValueError("fit: no sequence")
        D = float(discount)
        tables = [{} for _ in range(N)]
        for n in range(N):
            tot, kinds = {}, {}
            for g, c in cnt[n].items():
                tot[g[:-1]] = tot.get(g[:-1], 0) + c
                kinds[g[:-1]] = kinds.get(g[:-1], 0) + 1
            bow = {h: D * kinds[h] / tot[h] for h in tot}
            if n == 0:
                for w in [i for i in range(V) if i != blank] + [eos]:
                    tables[0][(w,)] = (math.log(max(cnt[0].get((w,), 0) - D, 0.0) / tot[()] + bow[()] / V), 0.0)
                tables[0][(bos,)] = (-99.0 * _LN10, 0.0)
            else:
                for h, b in bow.items():                 # the context's own entry carries its back-off weight
                    tables[n - 1][h] = (tables[n - 1][h][0], math.log(b))
                lower = cls(V, n, tables[:n], blank)
                for g, c in cnt[n].items():
                    h = g[:-1]
                    tables[n][g] = (math.log((c - D) / tot[h] + bow[h] * math.exp(lower._lookup(h[1:], g[-1]))), 0.0)
        return cls(V, N, tables, blank)

    # ---- the automaton --------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_tables(cls, logp, next, final, start=0, blank=0):
        """A compiled model straight from automaton tables (logp [S, V], next [S, V], final [S]): any deterministic automaton."""
        logp = torch.as_tensor(logp, dtype=torch.float32).contiguous()
        next = torch.as_tensor(next, dtype=torch.int32).contiguous()
        final = torch.as_tensor(final, dtype=torch.float32).contiguous()
        if logp.dim() != 2 or next.shape != logp.shape or final.shape != logp.shape[:1] or not 0 <= int(start) < max(logp.shape[0], 1):
            raise ValueError("from_tables: logp [S, V], next [S, V], final [S] and 0 <= start < S are required")
        self = cls(logp.shape[1], 1, None, blank)
        self.logp, self.next, self.final, self.start = logp, next, final, int(start)
        return self

    def compile(self):
        """Resolve the back-off into the automaton of the module's docstring; returns self."""
        if self.ngrams is None:
            return self
        V, N, eos = self.vocab_size, self.order, self.eos
        states = [()] + sorted((g for t in self.ngrams[:N - 1] for g in t if g[-1] != eos), key=lambda g: (len(g), g))
        S = len(states)
        if S * V > MAX_CELLS:
            raise ValueError(f"compile: {S} states x {V} labels is above the limit of 2^28 table cells")
        idx = {s: i for i, s in enumerate(states)}

        def home(ctx):                                   # the state whose row an unlisted context shares: its longest listed suffix
            while ctx not in idx:
                ctx = ctx[1:]
            return idx[ctx]

        kids = {}                                        # context -> its listed n-grams
        for t in self.ngrams[1:]:
            for g, (p, _) in t.items():
                kids.setdefault(g[:-1], []).append((g, p))
        lp = np.full((S, V + 2), -np.inf)                # columns V and V + 1: <s> (never predicted) and </s>
        nx = np.zeros((S, V), dtype=np.int64)
        for g, (p, _) in self.ngrams[0].items():
            lp[0, g[0]] = p
        for c in range(V):
            nx[0, c] = idx.get((c,), 0)
        for i in range(1, S):                            # by rising length, so the suffix' row is final: back off to it, then the
            s = states[i]                                # n-grams listed after s replace its values and, where they are states, lead on
            j = home(s[1:])
            lp[i] = self.ngrams[len(s) - 1][s][1] + lp[j]
            nx[i] = nx[j]
            for g, p in kids.get(s, ()):
                lp[i, g[-1]] = p
                if g in idx:
                    nx[i, g[-1]] = idx[g]
        lp[:, self.blank] = 0.0
        nx[:, self.blank] = np.arange(S)
        self.states = states
        self.logp = torch.from_numpy(lp[:, :V].astype(np.float32))
        self.next = torch.from_numpy(nx.astype(np.int32))
        self.final = torch.from_numpy((lp[:, eos] if self.has_eos else np.zeros(S)).astype(np.float32))
        self.start = idx.get((self.bos,), 0)               # order 1 has no context but the empty one
        return self

    @property
    def num_states(self):
        return 0 if self.logp is None else int(self.logp.shape[0])

    def to(self, device):
        """Move the automaton's three tensors; returns self."""
        if self.logp is None:
            raise RuntimeError("NGramLM.to: compile() first")
        self.logp, self.next, self.final = self.logp.to(device), self.next.to(device), self.final.to(device)
        return self
