"""How many index reads of a self-search does the matcher know the answer to?  For a gene set searched against itself, per seed shape: the positions
of the queries that start a seed and lie in a target that repeats its query (the chosen frame is frame 1 and fits one chunk), how many of them sit in a
bucket of the query index that holds exactly one entry - the matcher (seed_match, seeds.hip) takes that entry for the self entry without reading it when
the block carries PEP_SELF_SAFE - and how many hold a key no other position holds.  The library's hash_u64 and key (sum of reduced letters x base^i)
restated in numpy; no GPU.  The count is over ALL seed-starting positions of such a gene: the matcher leaves out the last, partial 32-byte block of
every stretch (about 3 % of the positions of a 334-residue gene).
python3 tools/self_singletons.py [n_genes] [gene_len] [--bucket-bits B] [--sensitive]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

PAD = 32                    # letters that never seed behind every protein: longer than any shape


def hash_u64(keys, bits):
    """seeds.hip: (k * 0x9E3779B97F4A7C15) >> (64 - bits), in 64-bit arithmetic"""
    with np.errstate(over='ignore'):
        return ((np.asarray(keys, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - bits)).astype(np.int64)


def bucket_bits_for(proteins):
    """pep_find_candidates: two buckets per packed query position (every sequence starts 16-aligned behind at least 16 bytes of padding), up to 2^25"""
    total = sum(((len(p) + 15) // 16) * 16 + 16 for p in proteins) + 32
    return max(10, min(25, int(np.ceil(np.log2(max(2 * total, 1))))))


def seed_table(proteins, offs, reduce, base):
    """keys of every position of the concatenated proteins (each followed by PAD never-seeding letters), which of them start a seed, and the
    protein of every position"""
    red = np.array([15 if r == 0xFF else r for r in reduce], dtype=np.uint64)
    parts, owner = [], []
    for g, p in enumerate(proteins):
        parts += [red[np.asarray(p, dtype=np.int64) & 31], np.full(PAD, 15, np.uint64)]
        owner.append(np.full(len(p) + PAD, g, np.int64))
    letters = np.concatenate(parts + [np.full(PAD, 15, np.uint64)])
    owner = np.concatenate(owner) if owner else np.zeros(0, np.int64)
    n = len(owner)
    keys, valid, w = np.zeros(n, np.uint64), np.ones(n, bool), np.uint64(1)
    for o in offs:
        g = letters[o:o + n]
        valid &= g != 15
        keys += g * w
        w *= np.uint64(base)
    return keys, valid, owner


def count_shape(proteins, is_self, offs, reduce, base, bits):
    """(seed-starting self positions, of them in a bucket of one entry, of them with a key that occurs once among the queries' seeds)"""
    keys, valid, owner = seed_table(proteins, offs, reduce, base)
    k = keys[valid]
    b = hash_u64(k, bits)
    per_bucket = np.bincount(b, minlength=1 << bits)
    uniq, inv, per_key = np.unique(k, return_inverse=True, return_counts=True)
    mine = np.asarray(is_self, dtype=bool)[owner[valid]]
    return int(mine.sum()), int((per_bucket[b][mine] == 1).sum()), int((per_key[inv][mine] == 1).sum())


def count_shape_brute(proteins, is_self, offs, reduce, base, bits):
    """the same count, one position at a time with Python integers and dictionaries"""
    buckets, per_key, seeds = {}, {}, []
    for g, p in enumerate(proteins):
        for x in range(len(p)):
            letters = [reduce[int(p[x + o]) & 31] if x + o < len(p) else 0xFF for o in offs]
            if 0xFF in letters:
                continue
            key = sum(l * base ** i for i, l in enumerate(letters))
            b = ((key * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> (64 - bits)
            buckets[b] = buckets.get(b, 0) + 1
            per_key[key] = per_key.get(key, 0) + 1
            if is_self[g]:
                seeds.append((key, b))
    return len(seeds), sum(buckets[b] == 1 for k, b in seeds), sum(per_key[k] == 1 for k, b in seeds)


def query_proteins(seqs, table=11):
    """the queries of a gene set as the search sees them (the oracle's frame choice) and which of them frame 1 of the same gene repeats as ONE target"""
    from oracle import oracle as O
    prots, is_self = [], []
    for s in seqs:
        frame, aa = O.query_frame(s.decode() if isinstance(s, bytes) else s, table)
        prots.append(O.aa_codes(aa))
        is_self.append(frame == 1 and 0 < len(aa) and len(O.ref_chunks(aa)) == 1)
    return prots, is_self


def shapes_of(params):
    return [[int(params.offs[s][i]) for i in range(int(params.weight[s]))] for s in range(int(params.n_shapes))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('genes', nargs='?', type=int, default=10000)
    ap.add_argument('gene_len', nargs='?', type=int, default=1002)
    ap.add_argument('--bucket-bits', type=int, default=0)
    ap.add_argument('--sensitive', action='store_true')
    args = ap.parse_args()
    from peppan_amd import _native as N, synth
    names, seqs = synth.make_genes(args.genes, args.gene_len, seed=355)
    prots, is_self = query_proteins(seqs)
    p = N.default_params(45., 25., 10, 5, sensitive=args.sensitive)
    bits = args.bucket_bits or bucket_bits_for(prots)
    print('%d genes, %d of them repeated by their frame-1 target, 2^%d buckets' % (len(prots), sum(is_self), bits))
    print('shape              self positions   singleton bucket   share   unique key   share')
    for s, offs in enumerate(shapes_of(p)):
        n, single, unique = count_shape(prots, is_self, offs, list(p.reduce), int(p.base), bits)
        text = ''.join('1' if i in offs else '0' for i in range(offs[-1] + 1))
        print('%-18s %14d %18d %6.1f %% %11d %6.1f %%' % (text, n, single, 100. * single / max(n, 1), unique, 100. * unique / max(n, 1)))


if __name__ == '__main__':
    main()
