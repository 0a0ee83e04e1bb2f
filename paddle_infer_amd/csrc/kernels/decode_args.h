// Argument blocks of the single-launch decode entry points (piamd_decode_mega /
// piamd_decode_head_greedy; kernels and field semantics in decode_mega.hip). Plain C++ with no HIP
// header, like fa_args.h: ops/_lib.py mirrors MegaArgs and HeadArgs with ctypes and a host
// compiler checks the mirrors' layout against these definitions.
#pragma once

typedef unsigned short bf16_t;  // bf16 carried as raw bits (same typedef as common.h)

struct MegaLayer {
  const bf16_t *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2;
  bf16_t *kc, *vc;
  // int8 weight-only mode (MegaArgs.w8): the four weights above are int8 [out][in] and these
  // are their per-output-channel f32 scales (null otherwise)
  const float *sqkv, *so, *s1, *s2;
};

struct MegaArgs {
  const MegaLayer* layers;
  int nl;
  int maxS;
  int nsplit;
  int act;  // 0 gelu (erf), 1 gelu (tanh)
  float eps;
  float scale_log2;
  const bf16_t* resid;  // [E] input residual (embedding output)
  bf16_t* rbuf;         // [2·nl][E] residual after each out / FFN2 phase; the last row is the output
  float* qn;            // [nl][HQ·D] q + bias
  float* kvn;           // [nl][2·HK·D] new k, v (+bias, bf16-rounded)
  float* part;          // [nl][pstride_l] attention partials [HQ][nsplit][PSTRIDE]
  bf16_t* h;            // [nl][F] FFN hidden
  unsigned* bar;        // barrier words (BAR_WORDS; zero before the first launch, re-zeroed by each)
  int* err;             // number of launches in which a grid barrier timed out
  const int* pos;       // [1] cache slot of the new token
  unsigned long long* trace;  // nullable: [NWG][5·nl][4] wall-clock (100 MHz): phase start,
                        // prologue done, GEMV done, barrier arrival
  int late_dma;         // bit 0: the FFN phases issue the next slice only after their GEMV; bit 1:
                        // attention workgroups queue their FFN1 head in the out prologue instead
                        // of at the end of the attention phase; bit 2: the FFN2 slice head is
                        // touched right behind the FFN1 head (decode_mega_kernel; A/B knobs)
  int loader;           // must be 0 (the retired dedicated-loader variant; field kept for the ABI)
  int rot;              // rotary dims: 0 or D (whole head)
  int neox;             // 1: rotate-half (NeoX), 0: interleaved pairs (GPT-J)
  float log2_base;      // log2 of the rotary base
  int w8;               // weight format: 0 bf16, 1 int8, 2 int4 weight-only (MegaLayer scales)
  int nb;               // batch rows per step (1, 2 or 4): resid / rbuf / qn / kvn / part / h hold
                        // nb rows per slot, pos nb entries, the caches are [rows][HK][maxS][D]
  int mm;               // 1 = MFMA GEMV phases, 0 = VALU (MegaCfg MM; the instantiated variant)
};

struct HeadArgs {
  const bf16_t *y, *g, *b;  // [E] final residual, final-LN gamma / beta
  float eps;
  int V;                    // vocabulary rows of `w`
  const bf16_t* w;          // [V][E] LM head
  unsigned long long* best;  // 8 words, 256-B apart (zero before the first launch)
  unsigned* cnt;            // 9 words, 256-B apart (zero before the first launch)
  long long* out;           // &out[0, t]
  unsigned char* done;      // [1] bool
  long long eos;            // < 0: no EOS
  long long pad;
  int* pos;                 // [1] slot of the token just decoded; advanced by one
  long long* tok;           // [1] chosen token (pad-masked)
  const bf16_t* wemb;       // [V][E] word embedding
  const bf16_t* pemb;       // [P][E] learned position embedding
  int P;
  bf16_t* resid;            // [E] next step's embedding output (written when pos + 1 < P)
};
