"""Inputs shared by tests/test_text_utf8_host.py and tests/test_gpu_text_utf8.py: raw texts with
2-, 3- and 4-byte characters around the wordset's tokens, and the packing of already normalized
texts into the layout of dice_batch_upload_text / dice_batch_upload_text_utf8."""
import random

import numpy as np

NON_ASCII = ('é', 'ü', '许可', '😀')     # 2, 2, 3 + 3 and 4 bytes of UTF-8
_WORDS = ('permission', 'is', 'hereby', 'granted', 'free', 'of', 'charge', 'users', 'software', 'class', 'its',
          'licensor', 'notice', 'warranty', 'liability', 'as', 'distribute', 'copies', 'terms', 'x', 'ss')
_SEPS = (' ', ' ', ' ', '\n', ', ', '. ', ' - ')


def fuzz_texts(n=300, seed=20250202):
    """``n`` raw texts: plain words mixed with words that have a non-ASCII character before, inside or
    after them, next to the possessive suffixes the wordset regex consumes ('s, s'), and alone."""
    rng = random.Random(seed)
    shapes = (lambda w, u: w, lambda w, u: w, lambda w, u: w,
              lambda w, u: u + w, lambda w, u: w + u, lambda w, u: w[:len(w) // 2] + u + w[len(w) // 2:],
              lambda w, u: w + "'s" + u, lambda w, u: u + w + "'s", lambda w, u: w + u + "'s",
              lambda w, u: "users'" + u, lambda w, u: u + "s'" + w, lambda w, u: w + "s'" + u + 's',
              lambda w, u: u, lambda w, u: u + u + u, lambda w, u: u + "'s", lambda w, u: w + "'" + u + "s'")
    out = []
    for _ in range(n):
        toks = [rng.choice(shapes)(rng.choice(_WORDS), rng.choice(NON_ASCII)) for _ in range(rng.randint(1, 90))]
        out.append(''.join(t + rng.choice(_SEPS) for t in toks))
    return out


def to_x80(s: str) -> bytes:
    """The one-byte-per-character form of lh_normalize_files: every non-ASCII character as 0x80."""
    return bytes(c if c < 0x80 else 0x80 for c in map(ord, s))


def pack(texts, fill=0xFF, slack=48, exact_end=False, gap=0):
    """texts (bytes) at 16-byte aligned offsets, ``gap`` extra 16-byte groups between files, every
    byte outside a file ``fill``; ``exact_end`` cuts the buffer at the last file's last byte
    (text_bytes = offsets[-1] + text_len[-1]). Returns (buffer uint8, offsets int64, text_len int32)."""
    tl = np.array([len(t) for t in texts], np.int32)
    step = (tl.astype(np.int64) + 15) // 16 * 16 + 16 * gap
    off = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64) if len(texts) else np.zeros(0, np.int64)
    buf = np.full(int(step.sum()) + slack, fill, np.uint8)
    for t, o in zip(texts, off.tolist()):
        buf[o:o + len(t)] = np.frombuffer(t, np.uint8)
    if exact_end:
        buf = buf[:int(off[-1]) + int(tl[-1])]
    return np.ascontiguousarray(buf), off, tl
