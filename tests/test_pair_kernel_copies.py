"""The headline kernel's row flavours run in sequence on one set of registers (extz2_pair.hip: lean_rows); what keeps the
compiler from folding the sequence back into an if / else chain is an empty asm on the row ranges.  Were it folded back, every
flavour would copy the thirty state registers in and out again and every result would still be right: so the copies are
counted, in the gfx950 code of the built library.

The bound: the chain costs the twelve flavours of extz2_pair_kernel<3,false,false> thirty copies in and thirty out each, 720
v_mov_b32 on top of what the function needs anyway (it had 1,211 as a chain and has 609 as a sequence); 900 lies between."""
import os
import shutil
import subprocess

MAX_V_MOV = 900
KERNEL = "_ZN3sdf17extz2_pair_kernelILi3ELb0ELb0EEEvPKNS_8PlanTaskEPKiPKjNS_6ScoreKEPhP10sdf_result"


def _tool(name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for d in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin"),
              os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    assert p, "%s of the ROCm LLVM tools not found" % name
    return p


def test_headline_kernel_keeps_its_state_in_place(tmp_path):
    from sedef_amd.build import LIB_PATH
    assert os.path.exists(LIB_PATH), "build the library first (python __graft_entry__.py)"
    fat, co, scratch = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co"), str(tmp_path / "lib.so")
    subprocess.check_call([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, LIB_PATH, scratch])
    subprocess.check_call([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    dis = subprocess.check_output([_tool("llvm-objdump"), "-d", "--disassemble-symbols=" + KERNEL, co], text=True)
    ops = [l.split()[0] for l in dis.split("\n") if l.startswith(("\t", " ")) and l.split()]
    assert len(ops) > 3000, "the kernel's code was not found in the library: %d instructions" % len(ops)
    n_mov = sum(op.startswith("v_mov_b32") for op in ops)
    print("v_mov_b32 of extz2_pair_kernel<3,false,false>: %d of %d instructions" % (n_mov, len(ops)))
    assert n_mov <= MAX_V_MOV, n_mov
