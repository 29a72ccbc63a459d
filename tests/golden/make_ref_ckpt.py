#!/usr/bin/env python3
"""Generates tests/golden/ref_ckpt/ from the reference's SHIPPED trained checkpoint (weights/stage-s5-curriculum).

usage: make_ref_ckpt.py <reference checkout>

Output = DATA only, as shipped: the `.index` SSTables and the object-graph shards (`.data-00000-of-00002`) of dynamics_model,
policy_net and value_net.  The policy / value TENSOR shards (`.data-00001-of-00002`, 1 MB each) are not copied: their tensors are
already committed in ref_trained_heads.npz, and tests/test_tf_checkpoint.py re-assembles each shard from them at the offsets its
index records.  shards.json holds the size and SHA-256 of every shipped tensor shard, so the re-assembled file is checked to be
the shipped one byte for byte.  (The trunk's tensor shard is not shipped by the reference.)
"""
import hashlib
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'ref_ckpt')


def main(ref_root):
    src = os.path.join(ref_root, 'weights', 'stage-s5-curriculum')
    os.makedirs(OUT, exist_ok=True)
    for ckpt in ('dynamics_model', 'policy_net', 'value_net'):
        for suffix in ('.index', '.data-00000-of-00002'):
            shutil.copyfile(os.path.join(src, ckpt + suffix), os.path.join(OUT, ckpt + suffix))
    shards = {}
    for ckpt in ('policy_net', 'value_net'):
        name = ckpt + '.data-00001-of-00002'
        raw = open(os.path.join(src, name), 'rb').read()
        shards[name] = dict(size=len(raw), sha256=hashlib.sha256(raw).hexdigest())
    with open(os.path.join(OUT, 'shards.json'), 'w') as f:
        json.dump(shards, f, indent=1)
        f.write('\n')
    print('wrote', OUT, sorted(os.listdir(OUT)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
