"""Register, spill, scratch and LDS use of the slot-walk kernels, from hipcc's kernel resource-usage remarks (no GPU needed):

    python tools/kernel_resources.py [csrc directory] > table.txt

compiles aggregate.hip, layer_fused2.hip and layer_fused3.hip for gfx950 (device code only) and prints one line per instantiation
of agg_fwd_kernel, agg_hub_kernel, layer_fused2_kernel and layer_fused3_kernel. A trailing `false` of the EE16 template parameter
 is dropped from the name, so that the table of a tree without that parameter can be compared line by line with
`diff`: profiles/ee16_kernel_resources.txt is that comparison for the commit that added the bf16 per-edge table.

    python tools/kernel_resources.py [csrc directory] dense.hip [more.hip ...] > table.txt

prints every kernel of the named translation units instead (profiles/candidates_kernel_resources.txt: dense.hip before and after
the candidate-list kernels were added to it)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ['aggregate.hip', 'layer_fused2.hip', 'layer_fused3.hip']
KERNELS = ('agg_fwd_kernel', 'agg_hub_kernel', 'layer_fused2_kernel', 'layer_fused3_kernel')
FIELDS = ['TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'SGPRs Spill', 'VGPRs Spill', 'LDS Size [bytes/block]']
SHORT = dict(zip(FIELDS, ['SGPRs', 'VGPRs', 'AGPRs', 'Scratch', 'SGPRSpill', 'VGPRSpill', 'LDS']))


def remarks(csrc, name, tmp):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    r = subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-c', '--cuda-device-only',
                        '-Rpass-analysis=kernel-resource-usage', '-o', os.path.join(tmp, name + '.o'), os.path.join(csrc, name)],
                       stderr=subprocess.PIPE, universal_newlines=True, check=True)
    return r.stderr


def parse(text):
    """{kernel name: {field: value}} of one translation unit's remarks."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r'remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass', line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def normalised(mangled):
    """(name without a trailing EE16 = false, is an EE16 = true instantiation). Itanium mangling: the template arguments end in
    ...Lb<0|1>E then E E v; a tree without the parameter is recognised by `has_ee16` = False of the caller."""
    m = re.match(r'^(.*)Lb([01])E(EEv.*)$', mangled)
    return (m.group(1) + m.group(3), m.group(2) == '1') if m else (mangled, False)


def table(csrc, has_ee16, files=None):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in files or FILES:
            for k, v in sorted(parse(remarks(csrc, name, tmp)).items()):
                if not files and not any(kk in k for kk in KERNELS):
                    continue
                shown, ee16 = normalised(k) if has_ee16 else (k, False)
                rows.append('%s%s  %s' % (shown, '  [EE16]' if ee16 else '', '  '.join('%s=%s' % (SHORT[f], v.get(f, '?')) for f in FIELDS)))
    return sorted(rows)


if __name__ == '__main__':
    files = [a for a in sys.argv[1:] if a.endswith(('.hip', '.cpp'))]
    dirs = [a for a in sys.argv[1:] if a not in files]
    csrc = dirs[0] if dirs else os.path.join(ROOT, 'kgc-gcn_amd', 'csrc')
    has = not files and 'EE16' in open(os.path.join(csrc, 'aggregate.hip')).read()
    print('\n'.join(table(csrc, has, files)))
