// media_amd/csrc/k_dec_ring.h -- the one piece of device work of the decoder's conceal mode (include/mi355x_h264_dec.h, "loss mode"):
// a stream that joins without an IDR picture decodes its first picture against reference pictures whose samples are all 128.
// k_dec_ring_fill writes those grey pictures: one launch per step, ahead of reconstruction, for all positions of the step that
// join, however many they are.  It is driven by the step's position table like the other kernels of a decoder step:
//   DecPos.w[6]  bit 0: the position joins; bits 4..7: the ring slots of its item to make grey
// blockIdx.z is the position, blockIdx.y the plane, blockIdx.x a run of 256 x 16 bytes of that plane.  A position that does not
// join, and the blocks of a chroma plane behind its end, leave at once.  Store-only: one 16-byte store per lane and slot.  A slot's
// plane is cw x ch (cw x ch / 4) bytes - the coded size, display and padding alike - and both are multiples of 64, every plane and
// slot starts on a multiple of 16: the stores are whole and aligned, and end where the slot's samples end, so the 256 zeroed bytes
// behind every slot, the other slots and the other items are never touched.
#pragma once

namespace h264 {

struct DecRingFill {
    uint8_t* base[3];            // the store's planes: [item][ring slot]
    size_t st_y, st_c;           // item strides
    size_t st_ring_y, st_ring_c; // ring-slot strides
    unsigned vec_y;              // 16-byte vectors of a luma slot (a chroma slot has a quarter of that)
    int nbuf;
};

__global__ __launch_bounds__(256) void k_dec_ring_fill(DecRingFill F, const DecPos* tab)
{
    const uint32_t w6 = (uint32_t)__builtin_amdgcn_readfirstlane((int)tab[blockIdx.z].w[6]);
    if (!(w6 & 1u)) return;
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)tab[blockIdx.z].w[0]) & 0xFFu;
    const int p = (int)blockIdx.y;
    const unsigned nvec = p ? F.vec_y >> 2 : F.vec_y;
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nvec) return;
    uint8_t* const plane = F.base[p] + (size_t)item * (p ? F.st_c : F.st_y) + (size_t)v * 16;
    const uint4 grey = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
    for (int s = 0; s < F.nbuf; s++)
        if ((w6 >> (4 + s)) & 1u) *(uint4*)(plane + (size_t)s * (p ? F.st_ring_c : F.st_ring_y)) = grey;
}

}  // namespace h264
