"""The distance the generated asm blocks keep behind v_dot4_u32_u8 (csrc/dice_program_gen.cpp, acc_block).

On gfx950 a VALU instruction other than a dot that reads or writes a dot's destination needs 3 wait
states behind it. The compiler inserts them in its own code but does not look inside an asm statement,
so the generator does: read here from the generated text, for the VALU program and the matrix-core
prologue, on corpora where count and bit dwords share a quad and where a count quad's block is followed
by other code. s_nop N counts N + 1 wait states, every other instruction one. No device is needed."""
import re

import pytest

from tests.test_program_compact_codegen import compact_source

DOT_WAIT = 3


def asm_blocks(src):
    """Per asm statement of the accumulate stages: its instructions as (opcode, operand list)."""
    out = []
    for body in re.findall(r'ACC_ASM_ONLY\(asm\("(.*?)" : ', src):
        out.append([(i.split()[0], [i.split()[1]] if i.startswith('s_nop') else re.findall(r'%\d+', i))
                    for i in body.split('\\n\\t')])
    return out


def check_blocks(blocks):
    """(dots, nops). Inside a block: a non-dot instruction that names a dot's destination comes at
    least DOT_WAIT wait states behind it. At its end: a block keeps DOT_WAIT wait states behind its
    last dot unless the next asm statement of the text is dots (and its own padding) alone."""
    n_dots = n_nops = 0
    for b, block in enumerate(blocks):
        pos, dot_at = 0, {}
        for op, args in block:
            if op == 's_nop':
                n_nops += 1
                pos += int(args[0]) + 1
                continue
            if op.startswith('v_dot4'):
                dot_at[args[0]] = pos
                n_dots += 1
            else:
                for a in args:
                    assert a not in dot_at or pos - dot_at[a] - 1 >= DOT_WAIT, (b, block)
            pos += 1
        if not dot_at:
            continue
        only_dots_next = b + 1 < len(blocks) and all(op.startswith('v_dot4') or op == 's_nop' for op, _ in blocks[b + 1])
        assert only_dots_next or pos - max(dot_at.values()) - 1 >= DOT_WAIT, (b, block)
    return n_dots, n_nops


def s_nop_lengths(src):
    return {int(n) for n in re.findall(r's_nop (\d+)', src)}


@pytest.mark.parametrize('stage', ['valu', 'mfma'])
@pytest.mark.parametrize('name', ['vendored', 'clones', 'count255', 'T2'])
def test_distance_behind_dots(name, stage, monkeypatch):
    from licensee_amd.corpus import TemplateCorpus
    from tests.test_gpu_corpus_sizes import corpus_of
    from tests.test_gpu_prog_index_in_den import _corpus
    monkeypatch.setenv('DICE_PROG_MATCH', stage)
    c = TemplateCorpus(corpus_of(2)) if name == 'T2' else _corpus(name)
    src = compact_source(c)
    n_dots, n_nops = check_blocks(asm_blocks(src))
    print(name, stage, 'dots', n_dots, 'nops', n_nops)
    assert n_dots > 0 and n_nops > 0
    # a nop that ends a block right behind a dot stands for all three wait states
    assert s_nop_lengths(src) <= {0, 1, 2} and 2 in s_nop_lengths(src)
