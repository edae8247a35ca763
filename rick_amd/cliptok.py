"""CLIP's byte-level BPE tokenizer (Radford et al., 2021) on the standard library: strings -> the id rows that
``ClipTextFeatures`` (rick_amd/cliptext.py) reads.  The vocabulary and the merges are the user's files; nothing is bundled.

    tok = ClipTokenizer.load('vocab.json', 'merges.txt', context=77)
    ids = tok(['a photo of a dog', 'a sketch'])             # int64 CPU [N, context]

The steps are those of the `transformers` library's ``CLIPTokenizer`` (verified against it on a tiny vocabulary,
tests/test_cliptext.py):

1. Unicode NFC;
2. every run of whitespace becomes one space;
3. lowercase;
4. pre-tokens, leftmost match of ``<|startoftext|>|<|endoftext|>|'s|'t|'re|'ve|'m|'ll|'d|\\p{L}+|\\p{N}|[^\\s\\p{L}\\p{N}]+``
   (whitespace separates and is dropped; a digit is a pre-token of its own).  ``unicodedata`` categories L* and N* stand in
   for \\p{L} and \\p{N}, ``str.isspace`` for \\s;
5. a pre-token's UTF-8 bytes, each mapped to its character in GPT-2's printable byte table;
6. ``</w>`` appended to the pre-token's last symbol;
7. merges by rank: the adjacent pair of the lowest rank, leftmost first, until no pair has a rank;
8. the row is ``[BOS] + ids + [EOT]``; a literal ``<|startoftext|>`` / ``<|endoftext|>`` in the text is that id.  As in
   `transformers`, the two are cut out of the raw text, exactly as spelt and wherever they stand, before step 1, and steps 1
   to 7 run on the pieces between them.  The two special alternatives of step 4's pattern then never decide anything: a
   spelling that only lowercasing turns into one of them (``<|ENDOFTEXT|>``) does match there, but the library's byte-level
   stage splits that pre-token again by GPT-2's pattern into ``<|``, ``endoftext``, ``|>``, which is what the other
   alternatives give, so step 4 here leaves the two out;
9. padded to `context` with `pad_id` (default 0, OpenAI's; `transformers` pads with EOT: under the causal mask and the
   first-maximum pooling rule every value gives the same embedding).

A row longer than `context` raises ValueError unless ``truncate=True``, which keeps the first context - 2 ids between BOS and
EOT, so EOT stays in the last position.  OpenAI's own tokenizer first runs ``ftfy.fix_text`` and ``html.unescape`` on the text;
neither is applied here.  A symbol that the vocabulary lacks raises (a complete CLIP vocabulary holds all 256 bytes in both
forms, so none is ever missing).
"""
import json
import re
import unicodedata

import torch

WHO = 'ClipTokenizer'
BOS, EOT = '<|startoftext|>', '<|endoftext|>'
CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")
END = '</w>'
_SPECIALS = re.compile('(' + '|'.join(re.escape(s) for s in (BOS, EOT)) + ')')


def byte_table():
    """GPT-2's byte -> printable character table: the printable Latin-1 bytes stand for themselves, the other 68 take the code
    points from 256 upwards in byte order."""
    keep = list(range(ord('!'), ord('~') + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    table, extra = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + extra)
            extra += 1
    return table


def normalise(text):
    """Steps 1 to 3."""
    text = unicodedata.normalize('NFC', text)
    out, space = [], False
    for ch in text:
        if ch.isspace():
            if not space:
                out.append(' ')
            space = True
        else:
            out.append(ch)
            space = False
    return ''.join(out).lower()


def pre_tokens(text):
    """Step 4 on normalised text: the list of pre-tokens in order.  The pattern's two special alternatives are not here: see
    step 8 of the module docstring."""
    kind = lambda ch: 's' if ch.isspace() else unicodedata.category(ch)[0] if unicodedata.category(ch)[0] in 'LN' else 'o'   # noqa: E731
    out, i, n = [], 0, len(text)
    while i < n:
        hit = next((s for s in CONTRACTIONS if text.startswith(s, i)), None)
        if hit is None:
            k = kind(text[i])
            if k == 's':
                i += 1
                continue
            j = i + 1
            if k != 'N':                                      # a run of letters, or of anything else that is no space
                while j < n and kind(text[j]) == k:
                    j += 1
            hit = text[i:j]
        out.append(hit)
        i += len(hit)
    return out


class ClipTokenizer:
    """CLIP's byte-level BPE; see the module docstring."""

    def __init__(self, vocab, merges, context=77, pad_id=0):
        """vocab: {symbol: id}; merges: a list of (left, right) pairs in rank order."""
        for s in (BOS, EOT):
            if s not in vocab:
                raise ValueError(f'{WHO}: the vocabulary has no {s!r}')
        if context < 2:
            raise ValueError(f'{WHO}: context must be at least 2 (BOS and EOT), got {context}')
        self.vocab = dict(vocab)
        self.rank = {tuple(m): r for r, m in enumerate(merges)}
        self.context, self.pad_id = int(context), int(pad_id)
        self.bos_id, self.eot_id = self.vocab[BOS], self.vocab[EOT]
        self._bytes = byte_table()
        self._cache = {}

    @classmethod
    def load(cls, vocab_json, merges_txt, context=77, pad_id=0):
        """vocab_json: the path of a JSON object {symbol: id}; merges_txt: the path of the merges, one 'left right' pair per
        line in rank order (a first line that starts with '#version' and empty lines are skipped)."""
        with open(vocab_json, encoding='utf-8') as f:
            vocab = json.load(f)
        merges = []
        with open(merges_txt, encoding='utf-8') as f:
            for n, line in enumerate(f):
                line = line.rstrip('\n')
                if not line.strip() or (n == 0 and line.startswith('#version')):
                    continue
                pair = line.split(' ')
                if len(pair) != 2:
                    raise ValueError(f'{WHO}: line {n + 1} of {merges_txt!r} is no pair of symbols: {line!r}')
                merges.append(tuple(pair))
        return cls(vocab, merges, context=context, pad_id=pad_id)

    def bpe(self, token):
        """Steps 5 to 7: one pre-token -> its list of symbols."""
        if token in self._cache:
            return self._cache[token]
        word = [self._bytes[b] for b in token.encode('utf-8')]
        word[-1] += END
        while len(word) > 1:
            best = min(range(len(word) - 1), key=lambda i: (self.rank.get((word[i], word[i + 1]), len(self.rank)), i))
            if (word[best], word[best + 1]) not in self.rank:
                break
            word[best:best + 2] = [word[best] + word[best + 1]]
        self._cache[token] = word
        return word

    def encode(self, text):
        """The ids of one string, without BOS, EOT and padding."""
        ids = []
        for n, piece in enumerate(_SPECIALS.split(text)):     # the odd pieces are the literal specials of the raw text
            if n % 2:
                ids.append(self.vocab[piece])
                continue
            for token in pre_tokens(normalise(piece)):
                for sym in self.bpe(token):
                    if sym not in self.vocab:
                        raise ValueError(f'{WHO}: symbol {sym!r} of {token!r} is not in the vocabulary')
                    ids.append(self.vocab[sym])
        return ids

    def __call__(self, texts, truncate=False):
        """A string or a list of strings -> int64 CPU [N, context]."""
        if isinstance(texts, str):
            texts = [texts]
        out = torch.full((len(texts), self.context), self.pad_id, dtype=torch.int64)
        for n, text in enumerate(texts):
            ids = self.encode(text)
            if len(ids) + 2 > self.context:
                if not truncate:
                    raise ValueError(f'{WHO}: {text!r} gives {len(ids) + 2} ids with BOS and EOT, the context is {self.context} '
                                     f'(truncate=True cuts it)')
                ids = ids[:self.context - 2]
            row = [self.bos_id] + ids + [self.eot_id]
            out[n, :len(row)] = torch.tensor(row, dtype=torch.int64)
        return out
