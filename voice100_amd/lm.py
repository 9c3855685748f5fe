"""A back-off n-gram language model over the acoustic model's own label ids, for the fused CTC prefix beam search (K25,
decode.ctc_beam_search(lm=...)).  Characters or phones: the space is a label like any other, so NGramLM has no lexicon and no word level;
the word level is WordNGramLM below, a second pass over the n-best list (K34).

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
compile() is Python over the states with numpy rows: seconds for 10^5 contexts.

WordNGramLM (K34, decode.rescore_nbest) is the same ARPA model over WORDS: a word is a maximal run of label ids other than `sep` inside a
hypothesis' length, a token is a word's tuple of ids or one of WordNGramLM.BOS / EOS / UNK (the strings "<s>", "</s>", "<unk>"), and
every word without a unigram is the one token UNK.  from_arpa, fit, to_arpa, log_prob and log_prob_eos mirror NGramLM's (the reader, the
estimator and the walk are NGramLM's own code).  A word vocabulary has no dense [S, V] automaton, so compile() lays out hash tables
that the kernel probes, all open addressing with linear probing, capacities powers of two, load <= 1/2 (table_bits: see compile):
    word ids      0 <unk>, 1 <s>, 2 </s>, then the vocabulary (the words with a unigram) sorted by spelling: 3, 4, ...
    pool          int64 [P]: the vocabulary's spellings, one after the other
    word_table    int32 [Cw, 4]: {word id, or -1 for an empty slot; offset of the spelling in the pool; its length; 0}, the home slot
                  hash(word) & (Cw - 1).  The hash only finds candidates: a slot is the word only if the length and every id agree
    ngram_table   int32 [sum over n of C_n (n + 2)]: per order n a table of C_n slots of n + 2 int32: the n word ids (the first one -1 for
                  an empty slot), then log p and the back-off weight as the bits of the float32 roundings of the float64 values; the
                  home slot is hash(the n ids) & (C_n - 1), and a slot is the n-gram only if all n ids agree
    meta          int64 [2 N], host memory: where each order's table begins inside ngram_table (in int32s), then its C_n
    hash          h = count * 0xD6E8FEB86659FD93; per element h = (h ^ element) * 0x9E3779B97F4A7C15, h ^= h >> 29 (all mod 2^64);
                  the slot is the low bits of h ^ (h >> 32).  Elements: a word's ids as they are (any int64: ids are only ever hashed
                  and compared, never an index), an n-gram's word ids
Table size: 8 bytes per label of the vocabulary's spellings, 32 bytes or more per word, 8 (n + 2) bytes or more per n-gram; 10^5 words
and 10^6 trigrams are some 50 MB.  Every table must stay below 2^31 int32s.  compile() is Python per entry: seconds for 10^5 entries."""
import math
import os

import numpy as np
import torch

__all__ = ["NGramLM", "WordNGramLM"]

MAX_ORDER = 8
MAX_CELLS = 1 << 28
_LN10 = math.log(10.0)


def _read_arpa(path_or_text, token):
    """The ARPA text as ([order] of {tuple of tokens: (log p, back-off weight)}, the <unk> unigram's log p or None), natural log.
    token(word) gives the token of an ARPA word, or None: n-grams that hold such a word are skipped (they still count against the
    header).  Malformed text: ValueError with the line number."""
    text = str(path_or_text)
    if "\n" not in text and "\\data\\" not in text:
        with open(os.fspath(path_or_text)) as f:
            text = f.read()

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
            g = tuple(token(w) for w in words)
            if any(t is None for t in g):
                continue
            if g in tables[-1]:
                raise bad(no, f"{' '.join(words)!r} is listed twice")
            if section > 1 and g[:-1] not in tables[-2]:
                raise bad(no, f"the context of {' '.join(words)!r} is not among the {section - 1}-grams")
            tables[-1][g] = (lp, bow)
    if not ended:
        raise bad(no, "\\end\\ is missing")
    return tables, unk


def _write_arpa(ngrams, order, name, eos):
    """The tables as ARPA text (log10, 9 decimals: 2.3e-9 in natural log); name(token) spells a token, rows sorted by their spelling's
    tokens where the tokens themselves do not sort."""
    out = ["\\data\\"] + [f"ngram {n + 1}={len(t)}" for n, t in enumerate(ngrams)]
    for n, table in enumerate(ngrams):
        out += ["", f"\\{n + 1}-grams:"]
        try:
            rows = sorted(table)
        except TypeError:
            rows = sorted(table, key=lambda g: [name(t) for t in g])
        for g in rows:
            lp, bow = table[g]
            row = f"{max(lp / _LN10, -99.0):.9f}\t" + " ".join(name(t) for t in g)
            if n + 1 < order and g[-1] != eos:
                row += f"\t{bow / _LN10:.9f}"
            out.append(row)
    return "\n".join(out + ["", "\\end\\", ""])


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
        V = len(symbols)
        bos, eos = V, V + 1
        tok = {s: i for i, s in enumerate(symbols) if i != blank}
        tok["<s>"], tok["</s>"] = bos, eos
        tables, unk = _read_arpa(path_or_text, tok.get)
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
        return _write_arpa(self.ngrams, self.order, name.__getitem__, self.eos)

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


def _hash64(count, elements):
    """The tables' hash (module docstring) of `count` and the elements, as a Python int below 2^32."""
    m = (1 << 64) - 1
    h = (count * 0xD6E8FEB86659FD93) & m
    for v in elements:
        h = ((h ^ (int(v) & m)) * 0x9E3779B97F4A7C15) & m
        h ^= h >> 29
    return (h ^ (h >> 32)) & 0xFFFFFFFF


def _capacity(entries, table_bits):
    """Slots for `entries` entries: the power of two >= 2 entries, or with table_bits the power of two >= max(2^table_bits, entries)."""
    need = max(2 * entries, 1) if table_bits is None else max(1 << int(table_bits), entries, 1)
    cap = 1
    while cap < need:
        cap <<= 1
    return cap


def _split_words(ids, sep):
    out, cur = [], []
    for x in ids:
        if int(x) == sep:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(int(x))
    return out + ([tuple(cur)] if cur else [])


class WordNGramLM:
    """A back-off n-gram model over words (module docstring): the second pass of decode.rescore_nbest (K34)."""
    BOS, EOS, UNK = "<s>", "</s>", "<unk>"
    UNK_ID, BOS_ID, EOS_ID, FIRST_WORD_ID = 0, 1, 2, 3

    def __init__(self, order, ngrams, sep=1, blank=0, symbols=None, unk_logp=None):
        self.order, self.sep, self.blank = int(order), int(sep), int(blank)
        self.ngrams = ngrams                             # [order] of {tuple of tokens: (logp, bow)}
        self.symbols = list(symbols) if symbols is not None else None
        self.unk_logp = unk_logp                         # compile() installs it where the model lists no <unk>
        self.has_bos, self.has_eos = (self.BOS,) in ngrams[0], (self.EOS,) in ngrams[0]
        self.pool = self.word_table = self.ngram_table = self.meta = None         # compile()
        self.word_ids = None

    # ---- the model as a function of the history ---------------------------------------------------------------------------------
    def start_history(self):
        return (self.BOS,) if self.has_bos else ()

    def token(self, word):
        """The token of a word (a sequence of ids; BOS / EOS / UNK stand for themselves): its tuple where it has a unigram, else UNK."""
        if isinstance(word, str):
            return word
        word = tuple(int(x) for x in word)
        return word if (word,) in self.ngrams[0] else self.UNK

    def words(self, ids):
        """The words of a sequence of ids: its maximal runs of ids other than sep, as tuples."""
        return _split_words(ids, self.sep)

    _lookup = NGramLM._lookup                            # the float64 back-off walk over the dictionaries

    def log_prob(self, history_words, word):
        """log p(word | history): history_words = start_history() + the words so far, each a tuple of ids."""
        return self._lookup(tuple(self.token(w) for w in history_words), self.token(word))

    def log_prob_eos(self, history_words):
        """log p(</s> | history), 0 where the model has no </s>."""
        return self._lookup(tuple(self.token(w) for w in history_words), self.EOS) if self.has_eos else 0.0

    # ---- ARPA text ------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arpa(cls, path_or_text, symbols, sep=1, blank=0, unk_logp=None):
        """NGramLM.from_arpa's format and errors.  An ARPA token is spelled in label ids through `symbols` (id -> one character; the
        entries at `blank` and `sep` spell nothing); <s>, </s> and <unk> are recognised; n-grams that hold a token with a character
        outside the symbols are skipped.  unk_logp (natural log): what compile() gives <unk> where the text does not list it."""
        char = {s: i for i, s in enumerate(symbols) if i != blank and i != sep}
        special = {"<s>": cls.BOS, "</s>": cls.EOS, "<unk>": cls.UNK}

        def token(w):
            if w in special:
                return special[w]
            ids = tuple(char.get(c) for c in w)
            return None if any(i is None for i in ids) else ids

        tables, _ = _read_arpa(path_or_text, token)
        return cls(len(tables), tables, sep, blank, symbols, unk_logp)

    def to_arpa(self, symbols=None):
        """The model as ARPA text (NGramLM.to_arpa's form); symbols default to those it was read with."""
        symbols = symbols if symbols is not None else self.symbols
        if symbols is None:
            raise ValueError("to_arpa: symbols (id -> character) are needed to spell the words")
        return _write_arpa(self.ngrams, self.order, lambda t: t if isinstance(t, str) else "".join(symbols[i] for i in t), self.EOS)

    # ---- the estimator --------------------------------------------------------------------------------------------------------------
    @classmethod
    def fit(cls, sequences, sep, order, discount=0.75, unk_logp=None):
        """NGramLM.fit on the words of the id sequences: the words, sorted, are numbered 1 .. W (0 plays the blank), the estimator runs
        on those numbers, and its tables are spelled back.  No <unk> comes out of it: pass unk_logp (or set the attribute) for compile()."""
        split = [_split_words(seq, int(sep)) for seq in sequences]
        vocab = sorted({w for s in split for w in s})
        num = {w: i + 1 for i, w in enumerate(vocab)}
        base = NGramLM.fit([[num[w] for w in s] for s in split], len(vocab) + 1, order, 0, discount)
        back = {i + 1: w for i, w in enumerate(vocab)}
        back[base.bos], back[base.eos] = cls.BOS, cls.EOS
        tables = [{tuple(back[t] for t in g): v for g, v in table.items()} for table in base.ngrams]
        return cls(order, tables, sep, 0, None, unk_logp)

    # ---- the tables of the kernel ---------------------------------------------------------------------------------------------------
    def compile(self, table_bits=None):
        """Lay out the tables of the module's docstring; returns self.  A model that lists no <unk> gets the unigram (unk_logp, no
        back-off weight); ValueError where unk_logp is None.  table_bits=k: every table has max(2^k, the power of two >= its entries)
        slots instead of load <= 1/2 -- k = 0 packs them as full as they go, so that probe chains grow long and wrap (tests)."""
        if (self.UNK,) not in self.ngrams[0]:
            if self.unk_logp is None:
                raise ValueError("compile: the model lists no <unk> and unk_logp is None")
            self.ngrams[0][(self.UNK,)] = (float(self.unk_logp), 0.0)
        vocab = sorted(g[0] for g in self.ngrams[0] if not isinstance(g[0], str))
        wid = {self.UNK: self.UNK_ID, self.BOS: self.BOS_ID, self.EOS: self.EOS_ID}
        wid.update({w: self.FIRST_WORD_ID + i for i, w in enumerate(vocab)})
        pool = np.array([i for w in vocab for i in w], dtype=np.int64)
        cw = _capacity(len(vocab), table_bits)
        wtab = np.zeros((cw, 4), dtype=np.int32)
        wtab[:, 0] = -1
        off = 0
        for w in vocab:
            slot = _hash64(len(w), w) & (cw - 1)
            while wtab[slot, 0] >= 0:
                slot = (slot + 1) & (cw - 1)
            wtab[slot] = (wid[w], off, len(w), 0)
            off += len(w)
        parts, meta, at = [], np.zeros(2 * self.order, dtype=np.int64), 0
        for n, table in enumerate(self.ngrams, 1):
            cap = _capacity(len(table), table_bits)
            tab = np.zeros((cap, n + 2), dtype=np.int32)
            tab[:, 0] = -1
            vals = tab[:, n:].view(np.float32)
            for g, (lp, bow) in table.items():
                key = [wid[t] for t in g]
                slot = _hash64(n, key) & (cap - 1)
                while tab[slot, 0] >= 0:
                    slot = (slot + 1) & (cap - 1)
                tab[slot, :n] = key
                vals[slot] = (lp, bow)                   # the float32 roundings of the float64 values
            parts.append(tab.reshape(-1))
            meta[n - 1], meta[self.order + n - 1] = at, cap
            at += tab.size
        if max(at, wtab.size, pool.size) >= 1 << 31:
            raise ValueError("compile: a table exceeds 2^31 - 1 elements (32-bit indices are the limit)")
        self.word_ids = wid
        self.pool = torch.from_numpy(pool if pool.size else np.zeros(1, dtype=np.int64))
        self.pool_len = int(pool.size)
        self.word_table = torch.from_numpy(wtab)
        self.ngram_table = torch.from_numpy(np.concatenate(parts))
        self.meta = meta
        return self

    def to(self, device):
        """Move the three tables (meta stays on the host); returns self."""
        if self.pool is None:
            raise RuntimeError("WordNGramLM.to: compile() first")
        self.pool, self.word_table, self.ngram_table = self.pool.to(device), self.word_table.to(device), self.ngram_table.to(device)
        return self
