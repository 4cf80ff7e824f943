#!/usr/bin/env python3
"""Old-versus-new floating-point census of the conv-block training kernels (a record of one comparison, not a tool of
the build).  In a directory that holds device-only assembly of the parent's two files and of block_train.hip,

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -x hip --cuda-device-only -S FILE -o NAME.s

as parent_ratio.s, parent_clf.s and new_block.s, it prints per pair of kernels whether the sequence of v_*_f32 / v_*_f64
instructions is the same, or their counts, and the counts (old/new where they differ).
"""
import collections
import re
import subprocess
def kernels(path):
    out = {}; name = None
    for line in open(path):
        m = re.match(r'^(_ZN4rgfm\w+):', line)
        if m: name = m.group(1); out[name] = []; continue
        if line.startswith('\t.section') or line.startswith('.Lfunc_end'):
            if line.startswith('.Lfunc_end'): name = None
            continue
        if name:
            t = line.strip().split()
            if t and re.match(r'^v_.*(f32|f64)', t[0]) : out[name].append(t[0])
    return out
def dem(n): return subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip().split('(')[0].replace('void ','').replace('rgfm::','',1)
P = {}; 
for f in ('parent_ratio.s','parent_clf.s'): P.update({dem(k): v for k, v in kernels(f).items()})
N = {dem(k): v for k, v in kernels('new_block.s').items()}
pairs = [('rt_norm_act_kernel','bt_act_kernel<rgfm::BtSilu, 1>'),('rt_norm_act_pool_kernel','bt_act_pool_kernel<rgfm::BtSilu, 1>'),
 ('rt_bn_bwd_part_kernel','bt_bn_bwd_part_kernel<rgfm::BtSilu, 1>'),('rt_bn_bwd_apply_kernel','bt_bn_bwd_apply_kernel<rgfm::BtSilu, 1>'),
 ('rt_unpool_kernel','bt_unpool_kernel<1>')]
for v in (1,4):
    pairs += [(f'ct_act_kernel<{v}>',f'bt_act_kernel<rgfm::BtRelu, {v}>'),(f'ct_act_pool_kernel<{v}>',f'bt_act_pool_kernel<rgfm::BtRelu, {v}>'),
      (f'ct_bn_bwd_part_kernel<{v}>',f'bt_bn_bwd_part_kernel<rgfm::BtRelu, {v}>'),(f'ct_bn_bwd_apply_kernel<{v}>',f'bt_bn_bwd_apply_kernel<rgfm::BtRelu, {v}>'),
      (f'ct_unpool_gate_kernel<{v}>',f'bt_unpool_kernel<{v}>')]
pairs += [('rt_bn_part_kernel','bt_bn_part_kernel'),('rt_bn_finalize_kernel','bt_bn_finalize_kernel'),('rt_bn_running_kernel','bt_bn_running_kernel'),
          ('rt_bn_bwd_finalize_kernel','bt_bn_bwd_finalize_kernel'),('rt_choice_kernel','bt_choice_kernel')]
for a, b in pairs:
    ca, cb = collections.Counter(P[a]), collections.Counter(N[b])
    same_seq = P[a] == N[b]
    print(f"{a:32s} -> {b:44s} {'same sequence' if same_seq else ('same counts' if ca == cb else 'DIFFERENT')}  " + ' '.join(f'{k}:{ca[k]}' + (f'/{cb[k]}' if ca[k]!=cb[k] else '') for k in sorted(set(ca)|set(cb))))
