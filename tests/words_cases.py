"""The device wordset scan (dice_words_kernel) judged by a plain regex: the reference, a buffer
builder that places files and fills the gaps, synthetic vocabularies, and inputs aimed at the
structural edges of the vocabulary table, the per-wave set and the chunked scan.

Reference (content_helper.rb:108-110 and nothing more): a file's tokens are RX.findall on its bytes
(for a bytes pattern \\w is ASCII, so bytes >= 0x80 separate tokens); its row is the set of tokens
that are vocabulary words, its field mask the set that are extra words, |W_F| = len(set(tokens)),
and status = 1 iff more than SET_MAX distinct tokens are neither (the header's contract); a flagged
file's row, |W_F| and mask are 0.

Nothing here imports oracle/, content_helper, native_host or GPU code. key_hash restates the
table's key hash in numpy; it was used offline to choose the literal words below, and
tests/test_words_cases.py re-proves every claimed property through dice_words_key_hash and
dice_vocab_geometry. No search runs at test time.
"""
from __future__ import annotations

import random
import re

import numpy as np

RX = re.compile(rb"(?:[\w/-](?:'s|(?<=s)')?)+")
SET_MAX = 192          # distinct non-vocabulary words the device set accepts
SET_SLOTS = 256
CHUNK = 1024           # bytes per staged chunk
BLOCK = 64             # bytes per block of the block loop
FAST_POS = 768         # run starts + ends a chunk may have on the fast path
Q_KEEP = 63            # queued tokens left after a flush
FILLS = {'zero': b'\0', 'apostrophes': b"s'"}


# ---- the key hash, restated --------------------------------------------------------------------

def _hash_matrix(a):
    """words_mix(host_key(w)) of equal-length words, [n, L] uint8 -> [n] uint64."""
    n, L = a.shape
    pad = np.zeros((n, 16), np.uint8)
    pad[:, :min(L, 16)] = a[:, :16]
    lo, hi = pad[:, :8].copy().view('<u8')[:, 0], pad[:, 8:].copy().view('<u8')[:, 0]
    tail = np.zeros(n, np.uint32)
    if L > 16:
        tail = np.full(n, 2166136261, np.uint32)
        for j in range(16, L):
            tail = (tail ^ a[:, j]) * np.uint32(16777619)
    p = (lo ^ (hi * np.uint64(0xC2B2AE3D27D4EB4F)) ^ (np.uint64(L) << np.uint64(56)) ^ tail.astype(np.uint64)) \
        * np.uint64(0x9E3779B97F4A7C15)
    return p ^ (p >> np.uint64(32))


def key_hash(words):
    """[n] uint64 key hashes of a list of bytes words."""
    out = np.zeros(len(words), np.uint64)
    by_len = {}
    for i, w in enumerate(words):
        by_len.setdefault(len(w), []).append(i)
    for L, idx in by_len.items():
        out[idx] = _hash_matrix(np.frombuffer(b''.join(words[i] for i in idx), np.uint8).reshape(len(idx), L))
    return out


def fnv1a(b):
    h = 2166136261
    for c in b:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


def geometry(n_total):
    """(buckets, id bits) of the table of n_total words: 8 slots a bucket, at most half full."""
    nb = 2
    while nb * 8 < 2 * n_total + 1:
        nb *= 2
    bits = 1
    while (1 << bits) <= n_total + 1:
        bits += 1
    return nb, bits


def bucket_and_tag(h, n_total):
    nb, bits = geometry(n_total)
    return int(h) & (nb - 1), (int(h) >> 40) & ((1 << min(24, 32 - bits)) - 1)


# ---- vocabularies, the reference, the buffer ---------------------------------------------------

class Vocab:
    """Vocabulary words in id order and extra words; the arrays of a 2-template corpus over them
    (the scan reads none of these: dice_create only needs a valid corpus)."""

    def __init__(self, words, extra=()):
        self.words, self.extra = [w for w in words], [w for w in extra]
        assert len(set(self.words) | set(self.extra)) == len(self.words) + len(self.extra) and len(self.extra) <= 64
        self.V = len(self.words)
        self.w64 = (self.V + 63) // 64

    def corpus_arrays(self):
        k = min(10, self.V)
        bits = np.zeros((2, self.w64), np.uint64)
        for t, ids in enumerate((range(k), range(self.V - k, self.V))):
            for i in ids:
                bits[t, i // 64] |= np.uint64(1 << (i % 64))
        size = np.full(2, k, np.uint32)
        return (bits, size, np.ones(2, np.uint32), np.full(2, 5, np.int32), (size * 6).astype(np.int32),
                np.zeros(2, np.uint8), self.V)


def reference(vocab, files):
    """(rows [n, w64] uint64, |W_F| [n] uint32, field masks [n] uint64, status [n] uint8)."""
    vid = {w.encode(): i for i, w in enumerate(vocab.words)}
    xid = {w.encode(): i for i, w in enumerate(vocab.extra)}
    n = len(files)
    rows = np.zeros((n, vocab.w64), np.uint64)
    wf, fm, st = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    for f, data in enumerate(files):
        toks = set(RX.findall(data))
        if sum(t not in vid and t not in xid for t in toks) > SET_MAX:
            st[f] = 1
            continue
        wf[f] = len(toks)
        for t in toks:
            if t in vid:
                rows[f, vid[t] // 64] |= np.uint64(1 << (vid[t] % 64))
            elif t in xid:
                fm[f] |= np.uint64(1 << xid[t])
    return rows, wf, fm, st


def build_buffer(files, fill, gaps=None, tail=0):
    """(text uint8, offsets int64, text_len int32): file i at a 16-byte aligned offset, gaps[i] further
    16-byte groups after it (default none), `tail` bytes after the last file (0: it ends exactly at
    text_bytes); every byte outside a file holds the repeated `fill` pattern."""
    gaps = gaps or [0] * len(files)
    off, at = [], 0
    for data, g in zip(files, gaps):
        off.append(at)
        end = at + len(data)
        at = (end + 15) // 16 * 16 + 16 * g
    size = (off[-1] + len(files[-1]) + tail) if files else tail
    text = np.frombuffer((fill * (size // len(fill) + 1))[:size], np.uint8).copy()
    for data, o in zip(files, off):
        text[o:o + len(data)] = np.frombuffer(data, np.uint8)
    return text, np.array(off, np.int64), np.array([len(d) for d in files], np.int32)


class Case:
    def __init__(self, name, vocab, files, gaps=None, tail=0):
        self.name, self.vocab, self.files, self.gaps, self.tail = name, vocab, [bytes(f) for f in files], gaps, tail


# ---- literals chosen offline with key_hash -----------------------------------------------------

# 25 words each whose home bucket at 8 buckets (16 <= n_total <= 31) is 2 / is 7 (the last), 3 of bucket 5
V1_B2 = ('acdehk aelmqg afacev aglmnj agzwrn aiulyx akdlug aklmmf alhrcz alrwrm apacuz aphufc apqceh aqmegz aqzioh '
         'attgdb augwdw auyocp awjxev awydfn axkeye axxgai azmazi azpjni aztxgt').split()
V1_B7 = ('aapzfw acbmkf aclpbj adcylz aenncw agaqdn agkglj ahkywj ahmrou aidunt akmffl ameccg andtqe aocvpm aqmcnu '
         'arhlct azhtdu bbzutv bcpyyd bdwavc becmcv behtnk bfkbek bgewwx bhmdij').split()
V1_OTHER = 'acjgrw agozjh anjyxc'.split()
# pairs with one home bucket (the third item) and one 24-bit tag at 2 buckets (n_total <= 7); fillers by bucket
V2_PAIRS = [('njvaoizc', 'zwodemkc', 1), ('hwbroqui', 'vuyjdexg', 1), ('cndtyvwl', 'qpldupzx', 0)]
V2_FILL = {0: ['aaaajmic', 'aaaiuwia', 'aaakumet'], 1: ['aaabwzgl', 'aaaeaajx', 'aaaecnao']}
# 192 words each whose home slot in the 256-slot set is 37 / is 250
S2_37 = ('aacyxde aaxqifg abvlccv afyrrez agunafu aiqgtie akglzxf akvzlcp alfdvdw alrdpgm ammqxkp aokxbry aowqmol aozmzjx '
         'apbpbma apyevtr atrcjzd avrbpfv avrbpoq awqveap axnmnnn ayqzrmh bazxepk bdbmoxj bdmdqlt bdwjgyj bfonxoj bgrakmp '
         'bhqnqqd bipfmvt blehvdz bmleund bnxowez bohfeqf bqvyzjr buaxiai buowntt buqvyxm bvjolad bvvofbh byekwrq bzyervd '
         'cavniaw cawkkir ccewdlc ccgvott cdeafyo cipqyrm cizmafx cogohbz cpoylty cqqtddv cqxpoaw ctymkxp cvwbjey cvyqxhh '
         'dadmgzh dbrqmqn dbutile ddijaal ddzuvwl dgmcjzb dkqmjcm dkvoqao dmuquuh dopzjlb dtdypgg dtqfifa dtzxqnu duzmodu '
         'dvyzukk dwglcmw dwlicti dwwuorl dwyvbri ecxrxxv eipbmaw ekhawva emczonp emjfwpu emjmfyx enunpft epozcth eptwctk '
         'epwhtdg eqmcren eukibhj euoycww evdetyw exexnmb fadtnae fawwbjh fbqpvnu fbyprpt fdmacgy fenmtey feoqeha fjtrloq '
         'flizpfr flmedui fmfqylu fmonwqe fqkcqkc fqqtebb frkmylj fvexrwt fxbpott gbmiflw gfmnakd ghbfbox ghbfbri gjyfrvy '
         'gkukuhz glxhvbk gqydxwo graexma gtbhofi gtpgtrf gtzhcrw gukfafy gwdgtjd gzkzklr hbckykq hbuqkcz hcfjbjh hcuvlpu '
         'hdzmqlh hennkgm hgpndpu hlhwvcx hluokcw hlxbdiy hmdcbdg hmnmebu hnmjhjq hnodlpu hqcdluz huatjaf hunqfdq huvozgu '
         'hvohmrc hwctcaa hxkguty iatiwud iewqnqc ihhuaif imefinh ipfceko ipiouae iqapmqo itgzljx ittgezf iubwqqa iudqujx '
         'iunghft iuqcuik iwlwfen iwqdcmb iwrflrr iwtwbrq ixbbahp izedcbc izhwbao jbxepio jbxeppf jcotbug jfhozhz jglplxa '
         'jhljqle jhljqnw jhoximf jhwxekm jiylnhg jljnyzv jljuhej jmggjej jmqvtkb jniwlub jnvmynd joueugy jrlmxwq jukfbqb '
         'jvkenoi jxodrro jyfayjf kbtalnx kexfkty keycmwh kgzfdiy kkexunf kkjuuny klppkom').split()
S2_250 = ('aapvwub aaxaiqa acfkzum acocqvh adtvoux aegnqxk ahdkock ahfqiht ajpovgd akfqclk alibnbt annzmkn aocxiam aoewttq '
          'apkmcca apthyty aqgwmii arvthak ayqzuon azcpnqb azgplge bayiumt bbhhhpr bcdrryd bedhdan bfyxxzv bfzlfor bhlqnhi '
          'bmbvnyn bmlerhg bqmlvhh btigkrp bverivh bwnyokd bwuwbvx bxkwgae bxowehv bxpddhq bxuqgyu bygqntm cancmef carhrzb '
          'cfwiyqm chautjt cijgpdb cizwktk cjzameh ckiitfd cldfyhp clhvzmk cllfuld cpfakcf cqleunc ctebudd ctvdvta cuvpfeu '
          'cvppihu cvzzlmr dbhwvaw deettnl dfepazm dgbwmvx dhnqlpu dlgxttf dmhfgio dobfdpc dpdfcpu dpexotf duftqbe dvcbfxo '
          'dvfuevg dvgbdbt dwzcjdq dxgajcq ebodnak ebrwmme edrfpqd eemzgjh efumybd egxuvfe ekjetzm endoyuw epewwat eqnuixm '
          'etmlkmo eurxzza evoahii exfhwyz exfxzlo exjxxoe fammaal faollhi fbndhgk fccbdoq feyuufb fhvybhj fjbxrgz fjmdxnj '
          'fkbbtuf fkfbrhc fkjybuj fkmuohn fkzbhcj foiopfd fpvvtqn ftchxkj futviah fycckua fznduok gafuelk gbpijvo gcqexip '
          'gfdxyzr glxlmhc gnbxhiw gqzqgcz gtxpnjo gveclby gwamvpr gwxkaey hapxoul hchwyhr heujgly hftwmdg hfxghcg hilbacv '
          'hknwdhq hmfraob hngdawh hnoidzx hptzttb hpywtuu hqkrtth hqqazzv hummfde hximbkg hzhoffl iadczqi ibnnqwp ichypcd '
          'icjcqpy idnmwnr ihalbbo iifxqrj iihruab ilhmhbc imaiztk imakbah imrvweq infwqmh iniufbj injrhpd iobqxga iouoedb '
          'ipwxxji iqlqmxh irpkpfa itcmzve itdahcr itladpw iuzejpn ivibulz ivzvacu iwbwapx iwkmpxf ixxdqoe iyiwyho jayanaq '
          'jbfoqix jdgglfp jdmqqvj jdoghkr jezhrlf jfeggtw jijbyku jinifed jnkztej jnvhbhd jodcddt jofrrzd jqbmmig jqcjoid '
          'jtuyobd jtwzbpb kalabpo katqami kcljvef kfubgod khhixlo khrjgrn kkfjgqi klhubxr').split()
# 24-byte words that share bucket and tag (2 buckets) with the token made of their first 16 bytes. (A
# 17-byte word cannot: one tail byte gives the tail hash too few values for the 24-bit tag to meet.)
V3_WORDS = ('commonprefix0123bar44ife', 'commonprefix0123t9p2nvy3')
# by tail length len - 16: two words with equal first 16 bytes and equal length that differ in their
# last 3 bytes only and share bucket and tag (2 buckets). Tails 3 and 31 end in a partial dword that
# holds every differing byte; 65 differs past the first 32 tail bytes. (Pairs that differ in the last
# byte alone, tails 1, 33 and 65 of that kind, do not exist in practice: the two tail hashes then differ
# by a small multiple of the FNV prime, and the tag does not meet.)
V4_PAIRS = {
    3: ('commonprefix0123qtr', 'commonprefix0123wrh'),
    31: ('commonprefix0123qvavlmphzbgjokdbabdzeqtfhkgzrhe', 'commonprefix0123qvavlmphzbgjokdbabdzeqtfhkgz358'),
    32: ('commonprefix0123exuwcjpmqqqbynxgjwebjqdwifnxxclu', 'commonprefix0123exuwcjpmqqqbynxgjwebjqdwifnxxni0'),
    33: ('commonprefix0123whauruaamikyfnihvdhcdhroleuufbgbz', 'commonprefix0123whauruaamikyfnihvdhcdhroleuufbw6v'),
    65: ('commonprefix0123hdummhmzfuahywcwwljzyqjfygnqghteqyrqlzfiqqcerwpyjiubeejduwjarcx8c',
         'commonprefix0123hdummhmzfuahywcwwljzyqjfygnqghteqyrqlzfiqqcerwpyjiubeejduwjarc1m6'),
}
# pairs with equal first 8 bytes, different later bytes and one home slot in the set: the set's second
# key word alone tells them apart
S3_SAME_SLOT = (('abcdefghak', 'abcdefghay'), ('abcdefghal', 'abcdefghbd'), ('abcdefghai', 'abcdefghbg'))
# two 8-byte tails with one 32-bit FNV-1a hash, behind one 16-byte prefix
S4_TAILS = ('oyeyvijj', 'yyrbdvjo')
PREFIX16 = 'commonprefix0123'

_AL = 'abcdefghijklmnopqrtuvwxyz'    # (no 's': apostrophes then never join)


def _words(n, k, seed):
    """n distinct k-letter words."""
    rng, out = random.Random(seed), []
    seen = set()
    while len(out) < n:
        w = ''.join(rng.choice(_AL) for _ in range(k))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def _join(words, sep=' '):
    return sep.join(words).encode()


# ---- the categories ----------------------------------------------------------------------------

def v1_spill():
    """17 vocabulary words of one home bucket (of 8): the chain fills two further buckets; home 7 wraps
    to bucket 0. Texts hold every word, and tokens outside the vocabulary whose home is the full bucket."""
    out = []
    for name, ws in (('V1-home2', V1_B2), ('V1-home7-wraps', V1_B7)):
        v = Vocab(ws[:17] + V1_OTHER)
        files = [_join(v.words), _join(ws[17:]), _join(ws[17:] + v.words[::-1] + ws[17:])]
        files += [w.encode() for w in ws[:17]]
        out.append(Case(name, v, files))
    return out


def v2_candidates():
    """Two vocabulary words with one home bucket and one tag, in slots (0, 1) and in slots (0, 4); a
    token outside the vocabulary with the bucket and tag of a vocabulary word."""
    (a1, a2, b), (c1, c2, _) = V2_PAIRS[0], V2_PAIRS[1]
    files = [a1, a2, a1 + ' ' + a2, a2 + ' ' + a1, c2, c2 + ' ' + c1, c1, ' '.join((a1, c2, a2, c1))]
    files = [f.encode() for f in files]
    return [Case('V2-low-low', Vocab([a1, a2, c1]), files),
            Case('V2-low-high', Vocab([a1] + V2_FILL[b] + [a2, c1]), files)]


def v3_edge16():
    """A 24-byte vocabulary word and the 16-byte token of its first 16 bytes (equal keys, bucket and
    tag: only the stored length tells them apart), and the roles swapped."""
    out = []
    for i, w in enumerate(V3_WORDS):
        p = w[:16]
        files = [f.encode() for f in (p, w, p + ' ' + w, w + '  ' + p, ' ' + p + 'x ' + p, w[:20] + ' ' + p)]
        out += [Case('V3-long-word-%d' % i, Vocab([w, 'filler']), files),
                Case('V3-short-word-%d' % i, Vocab([p, 'filler']), files)]
    return out


def v4_tail():
    """Per tail length, one word of the pair in the vocabulary and the other only in the text (both
    ways round), the token at every pos & 3."""
    out = []
    for tl, (u, v) in sorted(V4_PAIRS.items()):
        files = [(' ' * s + v + ' ' + ' ' * s + u + ' ' + v).encode() for s in range(4)]
        files += [(' ' * s + v).encode() for s in range(4)] + [(' ' * s + u).encode() for s in range(4)]
        out += [Case('V4-tail%d' % tl, Vocab([u, 'filler']), files),
                Case('V4-tail%d-swapped' % tl, Vocab([v, 'filler']), files)]
    return out


def v5_bits():
    """V = 130 (w64 = 3, 2 valid bits in the last word) and 64 extra words: one file per seam bit, one
    with everything; V = 64 without extra words."""
    words, extra = ['w%03d' % i for i in range(130)], ['e%02d' % i for i in range(64)]
    files = [words[i].encode() for i in (0, 31, 32, 63, 64, 127, 128, 129)]
    files += [extra[i].encode() for i in (0, 31, 32, 63)]
    files += [_join(words + extra), _join(extra + words[::-1] + ['other', 'words'])]
    w64 = ['w%03d' % i for i in range(64)]
    return [Case('V5-130-64', Vocab(words, extra), files),
            Case('V5-64-0', Vocab(w64), [w64[0].encode(), w64[31].encode(), w64[32].encode(), w64[63].encode(),
                                        _join(w64), b'e00 e63 ' + _join(w64)])]


def s1_capacity():
    """192 / 193 distinct words outside the vocabulary, in one chunk and over many, alone and with
    40 vocabulary words mixed in."""
    ws = _words(193, 3, 11)
    voc = ['v%02d' % i for i in range(40)]
    files = []
    for k in (192, 193):
        mixed = []
        for i, w in enumerate(ws[:k]):
            mixed.append(w)
            if i % 5 == 0 and i // 5 < 40:
                mixed.append(voc[i // 5])
        files += [_join(ws[:k]), _join(ws[:k], ' ' * 30), _join(mixed), _join(mixed, ' ' * 30),
                  _join(ws[:k] + ws[:k][::-1])]
    return [Case('S1', Vocab(voc, ['e0', 'e1']), files)]


def s2_probe_wrap():
    """192 words of one home slot (37; 250: the chain wraps past 255), each repeated later in the file."""
    return [Case('S2', Vocab(['vocab', 'word']),
                 [_join(S2_37 + S2_37), _join(S2_250 + S2_250[::-1]), _join(S2_250 + ['vocab'] + S2_250)])]


def s3_races():
    """One token 64 times in one lookup pass; keys that differ in the second half, in the length alone,
    in the tail alone; pairs that differ in the second key word and share a home slot; a long token
    repeated at another alignment and in another chunk."""
    p16 = PREFIX16
    long_a, long_b = p16 + 'tailtailtailA', p16 + 'tailtailtailB'
    files = [b'zqzqzq ' * 64, b'abcdefghX abcdefghY abcdefghX', _join([w for p in S3_SAME_SLOT for w in p + p[::-1]]),
             _join(S3_SAME_SLOT[0]), (p16 + ' ' + p16 + 'q ' + p16).encode(),
             (long_a + ' ' + long_b + '  ' + long_a).encode(),
             (' ' + long_a + ' ' * 1100 + long_a + '   ' + long_a + ' ' * 1000 + long_a).encode()]
    return [Case('S3', Vocab(['vocab', 'word']), files)]


def s4_fnv():
    """Two tokens of one length whose 16-byte prefixes are equal and whose tails have one FNV-1a hash:
    the only input on which the set's byte compare decides."""
    a, b = (PREFIX16 + t for t in S4_TAILS)
    return [Case('S4', Vocab(['vocab', 'word']),
                 [(a + ' ' + b).encode(), (b + '  ' + a + ' ' + b).encode(), (a + ' ' + a).encode()])]


_SINGLE = 'abcdefghijklmnopqrtuvwxyz0123456789_'


def f1_chunk(k, lead=b''):
    """A 1 KiB chunk: `lead`, then k single-character tokens, then separators."""
    body = lead + b''.join((_SINGLE[i % len(_SINGLE)] + ' ').encode() for i in range(k))
    return body + b' ' * (CHUNK - len(body))


def f1_position_area():
    """384 / 385 single-character tokens in one chunk (768 / 770 run starts and ends), alone and as
    chunk 1 of three with a token open from chunk 0 and one open into chunk 2."""
    files = [f1_chunk(384), f1_chunk(385)]
    for k in (383, 384):     # + the open token's end and the last token's start
        c1 = f1_chunk(k, b'yy ')[:CHUNK - 4] + b'zzzz'
        files.append(b' ' * (CHUNK - 10) + b'y' * 10 + c1 + b'zz after the chunk ' * 3)
    return [Case('F1', Vocab(['a', 'b', 'yyyyyyyyyyyy', 'zzzzzz'], ['c']), files)]


def f2_text():
    """Two chunks of "a b c ..." (32 token ends per 64-byte block), each forced through the block loop by
    one "x's'" (the token x's and an apostrophe) in place of its first two tokens, so its first block has
    31 ends; then 161 two-letter words. 39 single-character vocabulary words, 162 other words."""
    singles = b''.join((_SINGLE[i % len(_SINGLE)] + ' ').encode() for i in range(2 * CHUNK))
    chunk = b"x's'" + singles[:CHUNK - 4]
    return chunk + chunk + _join(_words(161, 2, 3)) + b' / - s'


def f2_queue():
    return [Case('F2', Vocab(list(_SINGLE) + ['/', '-', 's']), [f2_text()])]


def f2_queue_peak(data):
    """(peak fill, most ends in a block) of a model of the queue, not something a test can observe: every
    64-byte block pushes its token ends at once, then passes of 64 run until at most Q_KEEP remain."""
    nq = peak = 0
    ends = np.zeros(len(data) // BLOCK + 2, np.int64)
    for m in RX.finditer(data):
        if m.end() < len(data):
            ends[m.end() // BLOCK] += 1
    for e in ends:
        nq += int(e)
        peak = max(peak, nq)
        while nq > Q_KEEP:
            nq -= min(nq, 64)
    return peak, int(ends.max())


F3_LENGTHS = (1000, 2040, 2046, 2047, 2048, 2049, 2060, 3100)


def f3_rescan():
    """Runs of "s'" and "x's" of about 1,000, 2,040-2,060 and 3,100 bytes from file offsets 5 and 1,020
    (the serial re-scan leaves the two-chunk window), then text whose first token starts right after."""
    files = []
    for unit in (b"s'", b"x's"):
        for n in F3_LENGTHS:
            run = unit * (n // len(unit))
            for at in (5, 1020):
                head = (b'ab cd ' * 200)[:at - 1] + b' '
                files.append(head + run + b"''alpha beta's gamma")
                files.append(head + run + b" alpha users' x's")
    return [Case('F3', Vocab(['alpha', "beta's", 'ab', "x's"], ['gamma', 'cd']), files)]


F4_TOKEN = ('open' + 'abcdefghijklmnopqrtuvwxyz0123456789_-/' * 70)[:2500]
F4_LONG = ('vocabulary/word-' + 'zyxwvutrqponmlkjihgfedcba9876543210' * 70)[:2100]
F4_40 = 'a-vocabulary-word-of-exactly-40-bytes-xx'


def f4_open():
    """A 2,500-byte token from file offset 1,000 (its key is taken two chunks before its end), twice at
    different alignments, and with a twin that differs in byte 3; a 2,100-byte and a 40-byte
    vocabulary word at every shift from -41 to +1 around offsets 1,024 and 2,048."""
    t = F4_TOKEN.encode()
    twin = t[:3] + b'X' + t[4:]
    files = [b' ' * 1000 + t + b'    ' + t + b' end', b' ' * 1000 + t + b'    ' + twin + b' end',
             b' ' * 1000 + twin + b' ' + t, b'ab ' + t]
    for w in (F4_LONG, F4_40):
        for edge in (1024, 2048):
            for shift in range(-41, 2):
                at = edge + shift
                files.append((b'ab cd ' * 400)[:at - 1] + b' ' + w.encode() + b' ab end')
    return [Case('F4', Vocab([F4_LONG, F4_40, 'ab', 'end']), files)]


G_ENDS = (b'x', b"x'", b's', b"'", b'q')
G_LENGTHS = (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048)


def g_past_the_end():
    """Files of every length next to a 16-byte, chunk or window edge ending in x, x', s, ' and a word
    character, packed with no gap, the last ending exactly at text_bytes; a 3 KiB file followed by
    files of 0 and 1 byte (n = 1 and n = 5: a wave takes a second file with a stale window)."""
    v = Vocab(['ab', "cd's", 'x', 'q', "abs'"], ['s', "x's"])
    files = []
    for n in G_LENGTHS:
        for end in G_ENDS:
            if len(end) <= n:
                files.append((b"ab cd's " * 300)[:n - len(end)] + end)
    big = (b"users' x's ab cd's " * 200)[:3072]
    return [Case('G-edges', v, files), Case('G-stale-1', v, [big]),
            Case('G-stale-5', v, [big, b'', b's', big[:3071], b"'"])]


def n_files(n):
    """n files of mixed sizes 0-3 KiB."""
    rng = random.Random(n)
    pool = ['ab', "cd's", "users'", 'x', 'q', 'lorem', 'ipsum', 'dolor', "it's", 'a/b-c'] + _words(60, 5, 1)
    out = []
    for i in range(n):
        size = (0, 1, 17, 1024)[i % 4] if i % 7 == 0 else rng.randrange(0, 3072)
        out.append(_join([rng.choice(pool) for _ in range(size // 4 + 1)])[:size])
    return out


N_VOCAB = Vocab(['ab', "cd's", 'x', 'lorem', "it's", 'a/b-c'], ['q', 'ipsum'])
N_SIZES = (0, 1, 3, 4, 5)

L_W64 = 3936          # 4 waves x words_lds_per_wave(3936) = 160 KiB: the largest vocabulary accepted


def l_vocab(w64):
    return Vocab(['w%06d' % i for i in range(64 * w64)])


def l_largest():
    v = l_vocab(L_W64)
    ids = (0, 63, 64, v.V - 2, v.V - 1)
    files = [v.words[i].encode() for i in ids]
    files += [_join([v.words[i] for i in ids]), _join(v.words[1000:1300] + ['other']), b'w00000 w0000000 w251904']
    return Case('L', v, files)


def all_cases():
    """Every category but L (built on demand: a quarter of a million words)."""
    out = []
    for make in (v1_spill, v2_candidates, v3_edge16, v4_tail, v5_bits, s1_capacity, s2_probe_wrap, s3_races, s4_fnv,
                 f1_position_area, f2_queue, f3_rescan, f4_open, g_past_the_end):
        out += make()
    return out
