"""Is the device code of one HIP source the same in two versions?  Compares the gfx950 assembly kernel by kernel.

Compile both versions with build.py's flags plus `--cuda-device-only --save-temps` (each in a directory of its own, with the
headers of csrc/ beside it) and hand over the two `*-hip-amdgcn-amd-amdhsa-gfx950.s` files:
    python tools/tuning/isa_identity.py parent/q-hip-amdgcn-amd-amdhsa-gfx950.s new/q-hip-amdgcn-amd-amdhsa-gfx950.s
Per kernel (by mangled name) the text from its label to its end label, with comments and blank lines stripped and the
function's ordinal taken out of local labels (.LBB<n>_, .Lfunc_end<n>: they count functions in file order).  Prints the number
of kernels that differ and their names (profiles/r18/isa_identity.txt)."""
import re, subprocess, sys, hashlib
def funcs(p):
    out, cur, name = {}, [], None
    for l in open(p):
        l = re.sub(r'\s*;.*$', '', l.rstrip('\n'))
        if not l.strip(): continue
        l = re.sub(r'\.LBB\d+_', '.LBB_', l)       # labels carry the function's ordinal in the file
        l = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', l)
        m = re.match(r'^(_Z\w+):', l)
        if m and name is None:
            name = m.group(1); cur = []
        if name: cur.append(l)
        if l.startswith('.Lfunc_end') and name:
            out[name] = '\n'.join(cur); name = None
    return out
A, B = funcs(sys.argv[1]), funcs(sys.argv[2])
only_a, only_b = sorted(set(A) - set(B)), sorted(set(B) - set(A))
bad = [k for k in A if k in B and A[k] != B[k]]
n_instr = sum(len(v.split('\n')) for v in A.values())
print(f'kernels in the parent: {len(A)}   now: {len(B)}   only in the parent: {len(only_a)}   only now: {len(only_b)}')
print(f'kernels whose assembly (comments and blank lines stripped) differs: {len(bad)}   lines compared: {n_instr}')
h = hashlib.sha256('\n'.join(k + '\n' + A[k] for k in sorted(A)).encode()).hexdigest()
g = hashlib.sha256('\n'.join(k + '\n' + B[k] for k in sorted(B)).encode()).hexdigest()
print('sha256 over all kernels, sorted by name: parent', h[:16], ' now', g[:16])
if bad or only_a or only_b:
    dm = subprocess.run(['c++filt'], input='\n'.join(bad + only_a + only_b), capture_output=True, text=True).stdout.split('\n')
    for d in dm[:40]: print('  ', d.split('(')[0])
