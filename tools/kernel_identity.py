"""Machine-code identity of the kernels of two source trees (the check of a refactor that moves kernels between units: DESIGN sections 24, 27).
    python tools/kernel_identity.py TREE_A uad_gemm TREE_B uad_gemm,uad_conv5_f,uad_conv5_d
compiles the named csrc/ units of each tree device-only for gfx950 with the library's flags (each tree's own EXTRA_FLAGS), disassembles them, pairs the kernels
by demangled name and prints per kernel whether the instruction text (addresses stripped, alignment padding after the kernel's end ignored) and the resource
fields of the kernel metadata are identical.  Exit status 1 on any difference or unpaired kernel.  CPU only; it searches for nothing, it only diffs."""
import importlib.util, os, re, shutil, subprocess, sys, tempfile

LLVM = '/opt/rocm/lib/llvm/bin'
FIELDS = ('.vgpr_count', '.sgpr_count', '.agpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size', '.max_flat_workgroup_size', '.kernarg_segment_size')


def tool(name):
    return shutil.which(name) or os.path.join(LLVM, name)


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels_of(tree, units, tmp):
    """{demangled name: (instruction lines, resource fields)} over the units; a name met twice is kept as a list of two (reported as unpaired)"""
    pkg = os.path.join(tree, 'unsupervised_anomaly_detection_brain_mri_amd')
    spec = importlib.util.spec_from_file_location('b', os.path.join(pkg, 'build.py'))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    out = {}
    for u in units:
        obj = os.path.join(tmp, f'{abs(hash(tree))}_{u}.co')
        run(b._hipcc(), f'--offload-arch={b.ARCH}', '-O3', '-std=c++17', '--cuda-device-only', '--no-gpu-bundle-output', '-c',
            *b.EXTRA_FLAGS.get(u + '.hip', []), os.path.join(pkg, 'csrc', u + '.hip'), '-o', obj)
        meta, cur, col = {}, None, None
        for line in run(tool('llvm-readelf'), '--notes', obj).splitlines():      # kernel-level keys sit at the column of the first list item under amdhsa.kernels
            m = re.match(r'^(\s*)(- )?(\.\w+):\s*(\S*)$', line)
            if 'amdhsa.kernels:' in line: col = -1
            if not m or col is None: continue
            at = len(m.group(1)) + 2 * bool(m.group(2))
            if col == -1: col = at
            if at != col: continue
            if m.group(2): cur = {}
            cur[m.group(3)] = m.group(4)
            if m.group(3) == '.name': meta[m.group(4)] = cur
        text, sym = {}, None
        for line in run(tool('llvm-objdump'), '-d', obj).splitlines():
            m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
            if m: sym = m.group(1); text[sym] = []
            elif sym and line.strip(): text[sym].append(re.sub(r'//\s*[0-9A-Fa-f]+:', '//', line).strip())
        names = sorted(meta)
        for mangled, nice in zip(names, run(shutil.which('llvm-cxxfilt') or 'c++filt', *names).splitlines()):
            ins = text[mangled]
            while ins and ins[-1].split()[0] in ('s_nop', 's_code_end', '...'): ins.pop()      # alignment padding behind the kernel's end (objdump prints zero fill as "..."): depends on what follows it in its unit
            out.setdefault(nice, []).append((ins, tuple(meta[mangled].get(f) for f in FIELDS)))
    return out


def main():
    ta, ua, tb, ub = sys.argv[1], sys.argv[2].split(','), sys.argv[3], sys.argv[4].split(',')
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels_of(ta, ua, tmp), kernels_of(tb, ub, tmp)
    bad = 0
    for name in sorted(set(a) | set(b)):
        na, nb = len(a.get(name, [])), len(b.get(name, []))
        if na != 1 or nb != 1:
            print(f'UNPAIRED  {na} / {nb} definitions  {name}'); bad += 1
            continue
        (ia, ra), (ib, rb) = a[name][0], b[name][0]
        print(f"{'text identical' if ia == ib else 'TEXT DIFFERS  '}  {'resources identical' if ra == rb else 'RESOURCES DIFFER ' + str(ra) + ' ' + str(rb)}  {len(ia):6d} lines  {name}")
        bad += ia != ib or ra != rb
    print(f'{sum(map(len, a.values()))} kernels in A, {sum(map(len, b.values()))} in B, {bad} different or unpaired')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
