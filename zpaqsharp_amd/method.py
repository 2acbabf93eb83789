"""The reference's method strings (LibZPAQ.makeConfig, LibZPAQ.cs:388-1044): parse_args and make_config turn an
expanded method string `{x|s|0}N1,N2,...[{c|i|a|m|t|s|w}N...]...` into ZPAQL config text — `comp`/`hcomp` generated from
the component letters, and the PCOMP program of the chosen pre-processing level:

    level = N2 & 3:  0 none, 1 `lazy2` (bit-packed LZ77, LibZPAQ.cs:427-572), 2 `lzpre` (byte-aligned LZ77, :575-639),
                     3 `bwtrle` (inverse BWT, :642-795);   N2 in 4..7 adds E8E9 (the stand-alone E8E9 program :802-826)

expand_level is the step in front of it, LibZPAQ.compressBlock's choice of that string for a numeric method "LB,R,t"
(LibZPAQ.cs:124-283).

The PCOMP source texts below are the reference's programs (they are data the decoder must run, like the built-in model
bytecodes in models.py); the generator around them is this module's own code.  Context.compress_method and
compressor.compress(method=...) build their blocks from it; tools/methods.py re-exports it next to the CPU
pre-processors the tests compare the GPU against.
"""
from __future__ import annotations

import re
from typing import List, Tuple

from . import zpaql


def _lg(x: int) -> int:
    """floor(log2(x)) + 1 (LZBuffer.cs:116-126)."""
    return int(x).bit_length()


def _nbits(x: int) -> int:
    return bin(x).count("1")


def expand_level(method: str, n: int, hist=None) -> str:
    """The method string LibZPAQ.compressBlock makes of a numeric method "LB,R,t" for a block of n bytes (LibZPAQ.cs:124-283):
    L the level 0..9, B the block size digits (not used here), R the redundancy 0..255, t = 0..3 = binary, text, exe, both.
    Levels 5..9 need `hist`, the block's 4096 repetition-gap counts (Context.gap_hist_blocks, synth.gap_hist), for the
    periodic models of LibZPAQ.cs:257-280.  The text is the reference's, odd places included: level 4 with 24 <= type < 48
    runs `sasz` and "1c0,0,511" together without a comma."""
    if not method or not method[0].isdigit():
        raise ValueError("a numeric method starts with its level, a digit")
    arg0 = max(_lg(n + 4095) - 20, 0)
    commas, arg = 0, [0, 0, 0, 0]
    for ch in method[1:]:
        if commas >= 4:
            break
        if ch in ",.":
            commas += 1
        elif ch.isdigit() and commas < 4:
            arg[commas] = arg[commas] * 10 + int(ch)
    typ = 512 if commas == 0 else arg[1] * 4 + arg[2]
    level = int(method[0])
    doe8 = (typ & 2) * 2
    m = f"x{arg0}"
    htsz = f",{19 + arg0 + (arg0 <= 6)}"                # lz77 hash table size
    sasz = f",{21 + arg0}"                              # lz77 suffix array size
    if level == 0:
        return f"0{arg0},0"
    if level == 1:
        if typ < 40:
            return m + ",0"
        m += f",{1 + doe8},"
        if typ < 80:
            return m + "4,0,1,15"
        if typ < 128:
            return m + "4,0,2,16"
        if typ < 256:
            return m + "4,0,2" + htsz
        if typ < 960:
            return m + "5,0,3" + htsz
        return m + "6,0,3" + htsz
    if level == 2:
        if typ < 32:
            return m + ",0"
        m += f",{1 + doe8},"
        if typ < 64:
            return m + "4,0,3" + htsz
        return m + "4,0,7" + sasz + ",1"
    if level == 3:
        if typ < 20:
            return m + ",0"
        if typ < 48:
            return m + f",{1 + doe8},4,0,3" + htsz
        if typ >= 640 or typ & 1:
            return m + f",{3 + doe8}ci1"
        return m + f",{2 + doe8},12,0,7" + sasz + ",1c0,0,511i2"
    if level == 4:
        if typ < 12:
            return m + ",0"
        if typ < 24:
            return m + f",{1 + doe8},4,0,3" + htsz
        if typ < 48:
            return m + f",{2 + doe8},5,0,7" + sasz + "1c0,0,511"
        if typ < 900:
            return m + f",{doe8}ci1,1,1,1,2a" + ("w" if typ & 1 else "") + "m"
        return m + f",{3 + doe8}ci1"
    # 5..9: slow CM with lots of models, periodic ones from the gap histogram
    if hist is None:
        raise ValueError("levels 5 to 9 need the block's gap histogram (hist)")
    r = [int(x) for x in hist]
    if len(r) != 4096:
        raise ValueError("hist has 4096 counts")
    m += f",{doe8}"
    m += "w2c0,1010,255i1" if typ & 1 else "w1i1"
    m += "c256ci1,1,1,1,1,1,2a"
    n1 = n - r[1] - r[2] - r[3]
    for _ in range(2):
        period, score, t = 0, 0.0, 0
        j = 5
        while j < 4096 and t < n1:
            s = r[j] / (256.0 + n1 - t)
            if s > score:
                score, period = s, j
            t += r[j]
            j += 1
        if period > 4 and score > 0.1:
            m += f"c0,0,{999 + period},255i1"
            if period <= 255:
                m += f"c0,{period}i1"
            n1 -= r[period]
            r[period] = 0
        else:
            break
    return m + "c0,2,0,255i1c0,3,0,0,255i1c0,4,0,0,0,255i1mm16ts19t0"


def level_block_size(method: str) -> int:
    """The block size LibZPAQ.compress cuts its input into for a numeric method (LibZPAQ.cs:86-94): (2^20 << B) - 4096 with B
    the one or two digits after the level, at most 11, and 4 without them."""
    bs = 4
    if len(method) > 1 and method[1].isdigit():
        bs = int(method[1])
        if len(method) > 2 and method[2].isdigit():
            bs = bs * 10 + int(method[2])
        bs = min(bs, 11)
    return (0x100000 << bs) - 4096


def parse_args(method: str) -> Tuple[str, List[int], str]:
    """'x4,1,4,0,3,24ci1' -> ('x', [4,1,4,0,3,24,0,0,0], 'ci1')   (LibZPAQ.cs:394-416)."""
    typ = method[0]
    if typ not in "xs0i":
        raise ValueError("method must start with x, s, 0 or i")
    args = [0] * 9
    i, k = 1, 0
    while i < len(method) and k < 9 and (method[i].isdigit() or method[i] in ",."):
        if method[i].isdigit():
            args[k] = args[k] * 10 + int(method[i])
        else:
            k += 1
            if k < 9:
                args[k] = 0
        i += 1
    return typ, args, method[i:]


_E8E9_TAIL = """
    d=b b=0 do
      a=b a==d ifnot
        a+= 4 a<d if
          a=*b a&= 254 a== 232 if
            c=b b++ b++ b++ b++ a=*b a++ a&= 254 a== 0 if
              b-- a=*b
              b-- a<<= 8 a+=*b
              b-- a<<= 8 a+=*b
              a-=b a++
              *b=a a>>= 8 b++
              *b=a a>>= 8 b++
              *b=a b++
            endif
            b=c
          endif
        endif
        a=*b out b++
      forever
    endif
"""


def _pcomp_lazy2(args: List[int], doe8: bool) -> str:
    """LibZPAQ.cs:427-572."""
    rb = args[0] - 4 if args[0] > 4 else 0
    p = """pcomp lazy2 3 ;

  a> 255 if
"""
    if doe8:
        p += _E8E9_TAIL.replace("    d=b b=0 do", "    b=0 d=r 4 do")
    p += """
    a=0 b=0 c=0 d=0 r=a 1 r=a 2 r=a 3 r=a 4
    halt
  endif

  a<<=d a+=c c=a
  a= 8 a+=d d=a

  a=r 1 a== 0 if
    a= 1 r=a 2
    a=c a&= 3 a> 0 if
      a-- a<<= 3 r=a 3
      a=c a>>= 2 c=a
      b=r 3 a&= 7 a+=b r=a 3
      a=c a>>= 3 c=a
      a=d a-= 5 d=a
      a= 1 r=a 1
    else
      a=c a>>= 2 c=a
      d-- d--
      a= 3 r=a 1
    endif
  endif

  do a=r 1 a== 1 if a=d a> 2 if
    a=c a&= 1 a== 1 if
      a=c a>>= 1 c=a
      b=r 2 a=c a&= 1 a+=b a+=b r=a 2
      a=c a>>= 1 c=a
      d-- d--
    else
      a=c a>>= 1 c=a
      a=r 2 a<<= 2 b=a
      a=c a&= 3 a+=b r=a 2
      a=c a>>= 2 c=a
      d-- d-- d--
"""
    p += f"      a= {5 if rb else 2} r=a 1\n"
    p += """    endif
  forever endif endif
"""
    if rb:
        p += f"""
  a=r 1 a== 5 if a=d a> {rb - 1} if
    a=c a&= {(1 << rb) - 1} r=a 5
    a=c a>>= {rb} c=a
    a=d a-= {rb} d=a
    a= 2 r=a 1
  endif endif
"""
    p += """
  a=r 1 a== 2 if a=r 3 a>d ifnot
    a=c r=a 6 a=d r=a 7
    b=r 3 a= 1 a<<=b d=a
    a-- a&=c a+=d
"""
    if rb:
        p += f"    a<<= {rb} d=r 5 a+=d a-= {(1 << rb) - 1}\n"
    p += """    d=a b=r 4 a=b a-=d c=a

    d=r 2 do a=d a> 0 if d--
      a=*c *b=a c++ b++
"""
    if not doe8:
        p += " out\n"
    p += """    forever endif
    a=b r=a 4

    a=r 6 b=r 3 a>>=b c=a
    a=r 7 a-=b d=a
    a=0 r=a 1
  endif endif

  do a=r 1 a== 3 if a=d a> 1 if
    a=c a&= 1 a== 1 if
      a=c a>>= 1 c=a
      b=r 2 a&= 1 a+=b a+=b r=a 2
      a=c a>>= 1 c=a
      d-- d--
    else
      a=c a>>= 1 c=a
      d--
      a= 4 r=a 1
    endif
  forever endif endif

  a=r 1 a== 4 if a=d a> 7 if
    b=r 4 a=c *b=a
"""
    if not doe8:
        p += " out\n"
    p += """    b++ a=b r=a 4
    a=c a>>= 8 c=a
    a=d a-= 8 d=a
    a=r 2 a-- r=a 2 a== 0 if
      a=0 r=a 1
    endif
  endif endif
  halt
end
"""
    return p


def _pcomp_lzpre(args: List[int], doe8: bool) -> str:
    """LibZPAQ.cs:575-639."""
    p = """pcomp lzpre c ;

  a> 255 if
"""
    if doe8:
        p += _E8E9_TAIL
    p += f"""    b=0 c=0 d=0 a=0 r=a 1 r=a 2
  halt
  endif

  c=a a=d a== 0 if
    a=c a>>= 6 a++ d=a
    a== 1 if
      a+=c r=a 1 a=0 r=a 2
    else
      d++ a=c a&= 63 a+= {args[2]} r=a 1 a=0 r=a 2
    endif
  else
    a== 1 if
      a=c *b=a b++
"""
    if not doe8:
        p += " out\n"
    p += """      a=r 1 a-- a== 0 if d=0 endif r=a 1
    else
      a> 2 if
        a=r 2 a<<= 8 a|=c r=a 2 d--
      else
        a=r 2 a<<= 8 a|=c c=a a=b a-=c a-- c=a
        d=r 1
        do
          a=*c *b=a c++ b++
"""
    if not doe8:
        p += " out\n"
    p += """        d-- a=d a> 0 while

      endif
    endif
  endif
  halt
end
"""
    return p


def _pcomp_bwtrle(args: List[int], doe8: bool) -> str:
    """LibZPAQ.cs:642-795."""
    p = """pcomp bwtrle c ;

  a> 255 ifnot
    *b=a b++

  elsel

    b-- a=*b
    b-- a<<= 8 a+=*b
    b-- a<<= 8 a+=*b
    b-- a<<= 8 a+=*b c=a r=a 1

    a=b r=a 2

    do
      a=b a> 0 if
        b-- a=*b a++ a&= 255 d=a d! *d++
      forever
    endif

    d=0 d! *d= 1 a=0
    do
      a+=*d *d=a d--
    d<>a a! a> 255 a! d<>a until

    b=0 do
      a=c a>b if
        d=*b d! *d++ d=*d d-- *d=b
      b++ forever
    endif

    b=c b++ c=r 2 do
      a=c a>b if
        d=*b d! *d++ d=*d d-- *d=b
      b++ forever
    endif
"""
    if args[0] <= 4:
        p += """
    b=0 do
      a=c a>b if
        d=b a=*d a<<= 8 a+=*b *d=a
      b++ forever
    endif

    d=r 1 b=0 do
      a=d a== 0 ifnot
        a=*d a>>= 8 d=a
"""
        p += " *b=*d b++\n" if doe8 else " a=*d out\n"
        p += """      forever
    endif
"""
        if doe8:
            p += "\n" + _E8E9_TAIL
        p += """  endif
  halt
end
"""
    elif doe8:
        p += """
    a=r 2 a-- r=a 2

    c=0 d=r 1 do
      a=d a== 0 ifnot
        d=*d

        b=d a=*b a<<= 24 b=a
        a=r 4 r=a 5 a>>= 8 a|=b r=a 4

        a=c a> 3 if
          a=r 5 a&= 254 a== 232 if
            a=r 4 a>>= 24 b=a a++ a&= 254 a< 2 if
              a=r 4 a-=c a+= 4 a<<= 8 a>>= 8
              b<>a a<<= 24 a+=b r=a 4
            endif
          endif
        endif

        a=c a> 3 if a=r 5 out endif c++

      forever
    endif

    b=r 4
    a=c a> 3 a=b if out endif a>>= 8 b=a
    a=c a> 2 a=b if out endif a>>= 8 b=a
    a=c a> 1 a=b if out endif a>>= 8 b=a
    a=c a> 0 a=b if out endif

  endif
  halt
end
"""
    else:
        p += """
    d=r 1 do
      a=d a== 0 ifnot
        d=*d
        b=d a=*b out
      forever
    endif
  endif
  halt
end
"""
    return p


def make_config(method: str) -> Tuple[str, List[int]]:
    """Config text (with the $-arguments already substituted) and the nine numeric arguments of a method string."""
    from zpaqsharp_amd.models import E8E9_PCOMP
    typ, args, rest = parse_args(method)
    if typ == "0":
        return "comp 0 0 0 0 0 hcomp end\n", args
    level, doe8 = args[1] & 3, 4 <= args[1] <= 7
    membits = args[0] + 20
    if level == 1:
        hdr, pcomp = f"comp 9 16 0 {membits} ", _pcomp_lazy2(args, doe8)
    elif level == 2:
        hdr, pcomp = f"comp 9 16 0 {membits} ", _pcomp_lzpre(args, doe8)
    elif level == 3:
        hdr, pcomp = f"comp 9 16 {membits} {membits} ", _pcomp_bwtrle(args, doe8)
    else:
        hdr, pcomp = "comp 9 16 0 0 ", (E8E9_PCOMP.strip() + "\n" if doe8 else "end\n")

    # ---- context model (LibZPAQ.cs:835-1041): H[0..254] contexts, H[255..511] position of the last byte i-255,
    # M = last 64K bytes filling backward, C = pointer to the most recent byte; level 2 keeps its parse state in R1, R2
    ncomp, sb = 0, 5
    comp: List[str] = []
    hc: List[str] = ["hcomp", "c-- *c=a a+= 255 d=a *d=c"]
    if level == 2:
        hc.append(f"""  a=r 1 a== 0 if
    a= {111 + 57 * int(doe8)}
  else a== 1 if
    a=*c r=a 2
    a> 63 if a>>= 6 a++ a++
    else a++ a++ endif
  else
    a--
  endif endif
  r=a 1""")
    for m in re.finditer(r"([a-z])([0-9,.]*)", rest):
        if ncomp >= 254:
            break
        letter = m.group(1)
        v = [int(x) if x else 0 for x in re.split(r"[,.]", m.group(2))] if m.group(2) else []
        if letter == "c":                                  # context model: N1 limit / memory, N2 offset, N3.. masks
            v += [0] * (2 - len(v)) if len(v) < 2 else []
            sb = 11
            sb += _lg(v[1]) if v[1] < 256 else 6
            for x in v[2:]:
                if x < 512:
                    sb += _nbits(x) * 3 // 4
            sb = min(sb, membits)
            if v[0] % 1000 == 0:
                comp.append(f"{ncomp} icm {sb - 6 - v[0] // 1000}")
            else:
                comp.append(f"{ncomp} cm {sb - 2 - v[0] // 1000} {v[0] % 1000 - 1}")
            hc.append(f"d= {ncomp} *d=0")
            if 1 < v[1] <= 255:
                hc.append(f"a=c a&= {v[1] - 1} hashd" if _lg(v[1]) != _lg(v[1] - 1) else f"a=c a%= {v[1]} hashd")
            elif 1000 <= v[1] <= 1255:
                hc.append(f"a= 255 a+= {v[1] - 1000} d=a a=*d a-=c a> 255 if a= 255 endif d= {ncomp} hashd")
            for k, x in enumerate(v[2:]):
                line = "b=c " if k == 0 else ""
                if x == 255:
                    line += "a=*b hashd"
                elif 0 < x < 255:
                    line += f"a=*b a&= {x} hashd"
                elif 256 <= x < 512:
                    line += ("a=r 1 a> 1 if\n  a=r 2 a< 64 if\n    a=*b " + (f"a&= {x - 256}" if x < 511 else "") +
                             " hashd\n  else\n    a>>= 6 hashd a=r 1 hashd\n  endif\nelse\n  a= 255 hashd a=r 2 hashd\nendif")
                elif x >= 1256:
                    line += f"a= {((x - 1000) >> 8) & 255} a<<= 8 a+= {(x - 1000) & 255} a+=b b=a"
                elif x > 1000:
                    line += f"a= {x - 1000} a+=b b=a"
                if x < 512 and k < len(v[2:]) - 1:
                    line += "\nb++ "
                hc.append(line)
            ncomp += 1
        elif letter in "mts" and ncomp > int(letter == "t"):
            if len(v) < 1:
                v.append(8)
            if len(v) < 2:
                v.append(24 + 8 * int(letter == "s"))
            if letter == "s" and len(v) < 3:
                v.append(255)
            sb = 5 + v[0] * 3 // 4
            if letter == "m":
                comp.append(f"{ncomp} mix {v[0]} 0 {ncomp} {v[1]} 255")
            elif letter == "t":
                comp.append(f"{ncomp} mix2 {v[0]} {ncomp - 1} {ncomp - 2} {v[1]} 255")
            else:
                comp.append(f"{ncomp} sse {v[0]} {ncomp - 1} {v[1]} {v[2]}")
            if v[0] > 8:
                hc.append(f"d= {ncomp} *d=0 b=c a=0")
                w = v[0]
                while w >= 16:
                    hc.append("a<<= 8 a+=*b" + (" b++" if w > 16 else ""))
                    w -= 8
                if w > 8:
                    hc.append(f"a<<= 8 a+=*b a>>= {16 - w}")
                hc.append("a<<= 8 *d=a")
            ncomp += 1
        elif letter == "i" and ncomp > 0:                  # ISSE chain, context order growing by N1, N2, ...
            hc.append(f"d= {ncomp - 1} b=c a=*d d++")
            for k, x in enumerate(v):
                if ncomp >= 254:
                    break
                line = ""
                for j in range(x % 10):
                    line += "hash "
                    if k < len(v) - 1 or j < x % 10 - 1:
                        line += "b++ "
                    sb += 6
                line += "*d=a" + (" d++" if k < len(v) - 1 else "")
                hc.append(line)
                sb = min(sb, membits)
                comp.append(f"{ncomp} isse {sb - 6 - x // 10} {ncomp - 1}")
                ncomp += 1
        elif letter == "a":                                # MATCH
            if len(v) < 1:
                v.append(24)
            v += [0] * (3 - len(v))
            comp.append(f"{ncomp} match {membits - v[2] - 2} {membits - v[1]}")
            hc.append(f"d= {ncomp} a=*d a*= {v[0]} a+=*c a++ *d=a")
            sb = 5 + (membits - v[1]) * 3 // 4
            ncomp += 1
        elif letter == "w":                                # ICM-ISSE chain over word contexts
            dflt = [1, 65, 26, 223, 20, 0]
            v += dflt[len(v):]
            comp.append(f"{ncomp} icm {membits - 6 - v[5]}")
            for i in range(1, v[0]):
                comp.append(f"{ncomp + i} isse {membits - 6 - v[5]} {ncomp + i - 1}")
            hc.append(f"a=*c a&= {v[3]} a-= {v[1]} a&= 255 a< {v[2]} if")
            for i in range(v[0]):
                hc.append(("  d= %d" % ncomp if i == 0 else "  d++") + f" a=*d a*= {v[4]} a+=*c a++ *d=a")
            hc.append("else")
            for i in range(v[0] - 1, 0, -1):
                hc.append(f"  d= {ncomp + i - 1} a=*d d++ *d=a")
            hc.append(f"  d= {ncomp} *d=0\nendif")
            ncomp += v[0] - 1
            sb = membits - v[5]
            ncomp += 1
    text = hdr + str(ncomp) + "\n" + "\n".join(comp) + "\n" + "\n".join(hc) + "\nhalt\n" + pcomp
    return text, args


def model_of(method: str) -> Tuple[zpaql.Model, List[int]]:
    text, args = make_config(method)
    return zpaql.assemble(text), args


# ---------------------------------------------------------------------------------------------------------------------
# what the GPU pre-processors (zpaqhip_preprocess_blocks, zpaqhip_compress_method_blocks) accept
# ---------------------------------------------------------------------------------------------------------------------
def uses_sa(args: List[int]) -> bool:
    """The method strings whose LZBuffer searches a suffix array (LZBuffer.cs:153-158, :205)."""
    return (args[1] & 3) in (1, 2) and args[5] - args[0] >= 21


def uses_ht(args: List[int]) -> bool:
    """The level 1 / 2 method strings whose LZBuffer searches a hash table (LZBuffer.cs:153-158, :285-327)."""
    return (args[1] & 3) in (1, 2) and args[5] - args[0] < 21


HT_MAX_BUCKET_BITS = 6                                      # args[4] at most, on the hash-table route: 64 slots per search


def check_blocks(args: List[int], sizes, bwt: bool = False, sa: bool = False, ht: bool = False) -> None:
    """ValueError for what the C ABI refuses with ZPAQHIP_E_ARG: level 3 (BWT) unless `bwt` opts in, level 2 with args[2]
    outside 1..64, and a block longer than 2^(args[0] + 20) bytes at level 1 or 2 (its offsets would wrap the PCOMP's M),
    than 2^(args[0] + 20) - 4096 bytes at level 3 (compressBlock's own assertion, LibZPAQ.cs:289; it keeps the n + 5
    bytes inside bwtrle's M), or than 2^31 - 1 bytes.  With `sa` and a method that uses_sa (the suffix-array search):
    level 1 with args[2] < 4, args[2] or args[6] above 255, args[4] above 30 and a block longer than 2^24 bytes.
    With `ht` and a method that uses_ht (the hash-table search): args[3] != 0 (the second hash order, which compressBlock
    never writes and whose loop reads past the block's end), args[6] != 0 (look-ahead only acts through that loop), level 1
    with args[2] < 4, level 2 with args[2] < 2 (from 65 on level 2 does no search: all literals), args[2] > 255,
    args[0] > 11, args[4] > args[5] or > HT_MAX_BUCKET_BITS, args[5] > 30 and a block longer than 2^24 bytes."""
    level = args[1] & 3
    sa = sa and uses_sa(args)
    ht = ht and uses_ht(args)
    if ht:
        if args[3] != 0 or args[6] != 0:
            raise ValueError("the hash-table search takes neither a second hash order (args[3]) nor look-ahead (args[6])")
        if args[2] < (4 if level == 1 else 2) or args[2] > 255:
            raise ValueError(f"the hash-table search needs a minimum match length of {4 if level == 1 else 2} to 255, not {args[2]}")
        if args[0] > 11 or args[5] > 30 or args[4] > args[5] or args[4] > HT_MAX_BUCKET_BITS:
            raise ValueError(f"the hash-table search takes args[0] up to 11, args[5] up to 30 and args[4] up to args[5] and {HT_MAX_BUCKET_BITS}")
    if sa and level == 1 and args[2] < 4:
        raise ValueError(f"level 1 needs a minimum match length of 4 or more, not {args[2]}")
    if sa and (args[2] > 255 or args[6] > 255 or args[4] > 30):
        raise ValueError("the suffix-array search takes args[2] and args[6] up to 255 and args[4] up to 30")
    if level == 3 and not bwt:
        raise ValueError("BWT (level 3) pre-processing is not available on the GPU")
    if level == 2 and not 1 <= args[2] <= 64 and not ht:
        raise ValueError(f"level 2 needs a minimum match length of 1 to 64, not {args[2]}")
    if level:
        limit = min((1 << min(args[0] + 20, 62)) - (4096 if level == 3 else 0), (1 << 31) - 1, (1 << 24) if sa or ht else 1 << 31)
        for i, n in enumerate(sizes):
            if n > limit:
                raise ValueError(f"block {i} has {n} bytes; at level {level} a block holds at most {limit} "
                                 f"(2^(args[0] + 20){' - 4096' if level == 3 else ', 2^24 with the suffix-array search' if sa else ', 2^24 with the hash-table search' if ht else ''})")


def pre_bound(args: List[int], n: int) -> int:
    """Pre-processed bytes of an n-byte block at most (zh_pre.cpp pre_bound)."""
    level = args[1] & 3
    return (11 * n + 7) // 8 + 16 if level == 1 else 2 * n + 64 if level == 2 else n + 5 if level == 3 else n
