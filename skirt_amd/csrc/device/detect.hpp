// Instrument::detect on the device: detectSlot, frameAt, detectPeel (one lane, used by the event side)
// and detectKernel (the iteration's detection records).
// Compiles only where engine.hip includes it, inside its anonymous namespace (after Args and Shared).
#ifndef SKIRT_AMD_DEVICE_DETECT_HPP
#define SKIRT_AMD_DEVICE_DETECT_HPP

// Instrument::detect of one peel-off ray (FullInstrument.cpp:107-174 and the Simple/SED/Frame
// variants): what it adds to instrument slot `slot` (FullInstrument: 0 transparent, 1 direct stellar,
// 2 scattered stellar, 3 direct dust, 4 scattered dust, 5.. per scattering level); false if nothing.
// Lextf = L e^{-tau}.
__device__ __forceinline__ bool detectSlot(const DevInstr& ins, unsigned flags, int slot, double Lp, double Lextf,
                                           double& v) {
    v = Lextf;
    if (ins.kind != SKIRT_INSTR_FULL) return slot == 0;
    switch (rayCat(flags)) {
    case CAT_STAR_DIRECT:
        if (slot == 0) v = Lp;
        return slot <= 1;
    case CAT_STAR_SCATTERED: {
        const int lev = rayLevel(flags);
        return slot == 2 || (lev >= 1 && lev <= ins.levels && slot == 5 + lev - 1);
    }
    case CAT_DUST_DIRECT: return slot == 3;
    default: return slot == 4;
    }
}

// frame tally of an instrument: [lambda][pixel][slot] with the slots padded to slotStride (8 for a
// FullInstrument with up to 3 scattering levels), so that one detection's adds fall in one 64-byte line
__device__ __forceinline__ double* frameAt(const Args& a, const DevInstr& ins, int ell, int l, int slot) {
    return a.tally + ins.frameBase + ((long long)ell * ins.nx * ins.ny + l) * ins.slotStride + slot;
}

// Instrument::detect of one peel-off ray with optical depth tau by one lane: SEDs into `sed` (LDS sums
// of the workgroup) or, when null, the global tally; frames with f64 atomics
__device__ __forceinline__ void detectPeel(const Args& a, const DevInstr& ins, unsigned flags, int l, double Lp,
                                           double tau, double* sed) {
    const double Lextf = Lp * exp(-tau);
    const int nl = a.nlambda;
    const int ell = rayEll(flags);
    for (int slot = 0; slot < ins.nslots; slot++) {
        double v;
        if (!detectSlot(ins, flags, slot, Lp, Lextf, v)) continue;
        if (ins.kind != SKIRT_INSTR_FRAME) {
            if (sed) atomicAdd(&sed[ins.sedOff + slot * nl + ell], v);
            else atomicAddF64(a.tally + ins.sedBase + slot * nl + ell, v);
        }
        if (l >= 0 && ins.kind != SKIRT_INSTR_SED) atomicAddF64(frameAt(a, ins, ell, l, slot), v);
    }
}

// the detections of this iteration's peel-off rays (their optical depths are in the queue now).
// POL: a FullInstrument's three Stokes slots (DevInstr::stokes ..) receive Lextf Q, Lextf U, Lextf V of every
// detection, whatever its category (FullInstrument.cpp:136-141, 165-170); POL = false is the kernel as it was
template <bool POL>
__global__ void __launch_bounds__(kBlock) detectKernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const unsigned int nrays = CTR(a.ctr, CTR_DET + a.parity);  // this iteration's
    if (nrays == 0) return;
    Shared sh = stageTables(a, lds, STAGE_INSTR);
    const int copies = a.detCopies;
    for (int q = threadIdx.x; q < copies * a.nsed; q += blockDim.x) sh.sed[q] = 0.0;
    __syncthreads();
    unsigned int detects = 0;
    // eight lanes per ray, one per instrument slot (mod 8): the frame adds of one detection fall in one
    // 64-byte line (frameAt) and leave in one wave instruction, so they share one atomic request. Each
    // group of 8 lanes sums SEDs into its own LDS copy (up to 8 copies, as many as the LDS holds): the 8
    // rays of an instruction mostly hit the same few (slot, wavelength) sums, which one copy would
    // serialize. Without room for one copy (very many wavelengths x slots) the SED adds go to the tally.
    const int lane = threadIdx.x & 63, sub = lane & 7;
    double* sed = copies ? sh.sed + ((lane >> 3) & (copies - 1)) * a.nsed : nullptr;
    const unsigned int waves = gridDim.x * (blockDim.x / 64);
    const unsigned int wave = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    for (unsigned int base = wave * 8; base < nrays; base += waves * 8) {
        const unsigned int id = base + (lane >> 3);
        if (id >= nrays) continue;
        const DetRec d = a.det[id];
        const unsigned flags = d.flags;
        const DevInstr& ins = sh.instr[rayInstr(flags)];
        const int l = d.l, ell = rayEll(flags);
        const double Lp = d.Lp, Lextf = Lp * exp(-d.tau);
        for (int slot = sub; slot < ins.nslots; slot += 8) {
            double v;
            if (POL && ins.stokes > 0 && slot >= ins.stokes) {
                const DetPol q = a.detPol[id];
                v = Lextf * (slot == ins.stokes ? q.Q : (slot == ins.stokes + 1 ? q.U : q.V));
            } else if (!detectSlot(ins, flags, slot, Lp, Lextf, v)) continue;
            if (ins.kind != SKIRT_INSTR_FRAME) {
                if (sed) atomicAdd(&sed[ins.sedOff + slot * a.nlambda + ell], v);
                else atomicAddF64(a.tally + ins.sedBase + slot * a.nlambda + ell, v);
            }
            if (l >= 0 && ins.kind != SKIRT_INSTR_SED) atomicAddF64(frameAt(a, ins, ell, l, slot), v);
        }
        if (sub == 0) detects++;
    }
    // flush the per-workgroup SED sums
    __syncthreads();
    for (int q = threadIdx.x; copies && q < a.nsed; q += blockDim.x) {
        double v = 0.0;
        for (int g = 0; g < copies; g++) v += sh.sed[g * a.nsed + q];
        if (v != 0.0) {
            int ii = 0;
            while (ii + 1 < a.ninstr && sh.instr[ii + 1].sedOff <= q) ii++;
            atomicAddF64(a.tally + sh.instr[ii].sedBase + (q - sh.instr[ii].sedOff), v);
        }
    }
    const unsigned long long vals[8] = {0, 0, 0, 0, detects, 0, 0, 0};
    flushStats(a, vals);
}

#endif  // SKIRT_AMD_DEVICE_DETECT_HPP
