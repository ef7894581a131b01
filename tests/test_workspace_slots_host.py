"""The shared device workspace pep_ctx::ws is addressed by name only.  Read from the sources, no library loaded:

    no .hip or .h under peppan_amd/csrc indexes `ws`, or a `DevBuf *W` that aliases it, with an integer literal;
    PEP_WS_COUNT, the last enumerator of the PEP_WS_* map in common.h, is the dimension of pep_ctx::ws;
    every file that says `ctx->ws` holds its slots below the device-resident hit table with a static_assert on PEP_WS_HITS_OUT - but for the
    search pipeline itself (seeds.hip, sw.hip, trace.hip) and common.h, which owns the map; of those only trace.hip, which writes the table,
    and common.h may name PEP_WS_HITS_OUT in code."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'peppan_amd', 'csrc')
PIPELINE = ('seeds.hip', 'sw.hip', 'trace.hip', 'common.h')


def sources():
    names = sorted(n for n in os.listdir(CSRC) if n.endswith(('.hip', '.h')))
    assert 'common.h' in names and 'seeds.hip' in names and len(names) >= 25
    return {n: open(os.path.join(CSRC, n), encoding='utf-8').read() for n in names}


def without_comments(text):
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return '\n'.join(line.split('//', 1)[0] for line in text.split('\n'))


def test_no_slot_is_addressed_by_a_number():
    found = []
    for name, text in sources().items():
        for k, line in enumerate(text.split('\n'), 1):
            if re.search(r'\bws\s*\[\s*\d', line) or re.search(r'\bW\s*\[\s*\d', line):
                found.append('%s:%d: %s' % (name, k, line.strip()))
    assert not found, '\n'.join(found)


def ws_enum(common):
    """the PEP_WS_* enumerators of common.h in order -> [(name, value)]; an enumerator is a number, another enumerator or one more than the last"""
    body = re.search(r'enum\s+PepWsSlot\s*\{(.*?)\n\};', without_comments(common), flags=re.S).group(1)
    out, value = [], -1
    for item in (x.strip() for x in body.split(',')):
        if not item:
            continue
        m = re.fullmatch(r'(PEP_WS_\w+)(?:\s*=\s*(\w+))?', item)
        assert m, item
        value = value + 1 if m.group(2) is None else int(m.group(2)) if m.group(2).isdigit() else dict(out)[m.group(2)]
        out.append((m.group(1), value))
    return out


def test_the_map_ends_at_the_dimension_of_ws():
    common = sources()['common.h']
    slots = ws_enum(common)
    assert slots[-1][0] == 'PEP_WS_COUNT' and dict(slots)['PEP_WS_HITS_OUT'] == slots[-1][1] - 1
    assert max(v for _, v in slots) == slots[-1][1]                        # nothing above the count
    dim = re.findall(r'\bDevBuf\s+ws\s*\[\s*(\w+)\s*\]', without_comments(common))
    assert dim == ['PEP_WS_COUNT']


def test_every_user_of_ws_stays_below_the_hit_table():
    users = {n: without_comments(t) for n, t in sources().items() if 'ctx->ws' in t}
    assert set(PIPELINE[:3]) <= set(users) and len(users) >= 12
    for name, code in users.items():
        if name not in PIPELINE:
            assert re.search(r'static_assert\s*\([^;]*PEP_WS_HITS_OUT', code), '%s uses ctx->ws without a static_assert on PEP_WS_HITS_OUT' % name
    for name in ('seeds.hip', 'sw.hip'):
        assert 'PEP_WS_HITS_OUT' not in users[name], '%s names PEP_WS_HITS_OUT in code' % name
